"""-m gpu: the HIP DrMvsnet path through the C ABI (CallAsync / Ready / GetResult, dr_mvsnet.h:36-66) against
(a) the golden fixtures = outputs of the reference PyTorch model, and (b) the CPU oracle on seeded windows.

Tolerance (floating point, stated): the reference's own acceptance test passes at mean-abs error < 1e-2 for
stage-3 depth and confidence (dr_mvsnet.cpp:505-513).  We hold the HIP path to
    mean|depth - ref| < 1e-4 m,  mean|confidence - ref| < 1e-4,
    99.9 % of depth_dense pixels within 2e-3 m,  EVERY depth_dense pixel within 2 % of the depth range (5e-2 m at the
    windows used here: a hypothesis interval of the last stage is ~1e-2 m, so no pixel may jump planes by more than a few),
    filter-mask disagreement < 0.2 % of pixels
(fp32 reassociation in convolutions moves values by ~1e-5; the confidence index trunc(E[k]) and the exact
quantile threshold are discontinuous, so isolated pixels may flip -- counted, not hidden)."""
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "mvsnet_*.npz")))


def compare(out, ref, what="", max_err=5e-3):
    """The fp32 bounds every end-to-end case is held to.  max_err: no single pixel may be off by more than 5 mm (observed maximum over all
    fixtures: 6e-4 m; until round 4 this bound was 5e-2 m, 80 x the observed error -- a plane jump at an isolated pixel would have passed)."""
    d_err = np.abs(out.depth_dense - ref["depth_dense"])
    print("compare(%s): depth_dense mean %.2e max %.2e m" % (what, d_err.mean(), d_err.max()))
    assert d_err.mean() < 1e-4, f"{what} depth_dense mean err {d_err.mean()}"
    assert (d_err < 2e-3).mean() > 0.999, f"{what} depth_dense outliers {(d_err >= 2e-3).mean()}"
    assert d_err.max() < max_err, f"{what} depth_dense max err {d_err.max()} m"
    assert np.abs(out.confidence_dense - ref["confidence_dense"]).mean() < 1e-4
    flips = ((out.depth == 0) != (ref["depth"] == 0)).mean()
    assert flips < 2e-3, f"{what} mask flips {flips}"
    assert np.abs(out.depth - ref["depth"]).mean() < 1e-2 and np.abs(out.confidence - ref["confidence"]).mean() < 1e-2
    same = (out.depth == 0) == (ref["depth"] == 0)
    assert np.abs(out.depth - ref["depth"])[same].mean() < 1e-4
    # the four outputs are mutually consistent (cva_mvsnet.py:168-173)
    kept = out.depth != 0
    assert np.array_equal(out.depth[kept], out.depth_dense[kept])
    assert np.all(out.confidence[~kept] == 0)


def blob_for(g, trained_blob, tmp_path):
    from tandem_amd import weights as Wt
    planes = tuple(int(v) for v in g["planes"])
    if str(g["weights"]) == "trained":
        _, tens = Wt.read_blob(trained_blob)
    else:
        tens = Wt.random_state(planes, seed=7)
    va = bool(int(g["view_aggregation"])) if "view_aggregation" in g.files else True
    p = str(tmp_path / "w.tdmw")
    Wt.write_blob(p, tens, depth_num=planes, view_aggregation=va)
    return p


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p) for p in GOLD])
def test_golden_fixture_through_call_async(path, trained_blob, tmp_path):
    from tandem_amd.dr_mvsnet import DrMvsnet
    g = np.load(path)
    m = DrMvsnet(blob_for(g, trained_blob, tmp_path))
    bgrs = [np.ascontiguousarray(b) for b in g["bgrs"]]
    H, W = bgrs[0].shape[:2]
    m.CallAsync(H, W, len(bgrs), int(g["ref_index"]), bgrs, g["K"], list(g["c2ws"]), float(g["depth_min"]),
                float(g["depth_max"]), float(g["discard"]))
    out = m.GetResult()
    assert m.Ready()
    ref = {k: g[f"ref_s3_{k}"] for k in ("depth", "confidence", "depth_dense", "confidence_dense")}
    compare(out, ref, os.path.basename(path))
    for s in (1, 2):  # earlier stages (unfiltered) via the introspection hook
        d, c = m.stage_output(s)
        assert np.abs(d - g[f"ref_s{s}_depth_dense"]).mean() < 1e-4
        assert np.abs(c - g[f"ref_s{s}_confidence_dense"]).mean() < 1e-4
    m.close()


def test_full_size_window_against_oracle(trained_blob):
    """BASELINE config 2: 640x480, ref + 6 src, planes (48,32,8)."""
    from oracle import mvsnet_oracle as O
    from synth import scene
    from tandem_amd import weights as Wt
    from tandem_amd.dr_mvsnet import DrMvsnet
    meta, tens = Wt.read_blob(trained_blob)
    win = scene.make_window(480, 640, 7, seed=0)
    ref = O.forward(O.Weights(meta, tens), win["bgrs"], win["K"], win["c2ws"], win["ref_index"], win["depth_min"],
                    win["depth_max"], 10.0)
    m = DrMvsnet(trained_blob)
    for _ in range(2):  # second call re-uses the plan and must give the same answer
        m.CallAsync(480, 640, 7, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), win["depth_min"],
                    win["depth_max"], 10.0)
        out = m.GetResult()
        compare(out, ref, "full")
    assert abs((out.depth == 0).mean() - 0.10) < 1e-3  # discard_percentage = 10
    m.close()


def test_protocol_and_argument_errors(trained_blob):
    from synth import scene
    from tandem_amd import _lib
    from tandem_amd.dr_mvsnet import DrMvsnet
    win = scene.make_window(64, 96, 3, seed=1)
    m = DrMvsnet(trained_blob)
    args = (64, 96, 3, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), 0.5, 5.0, 2.5)
    m.CallAsync(*args)
    m.Wait()
    assert m.Ready()
    m.GetResult()
    with pytest.raises(_lib.DrError) as e:  # dr_mvsnet.cpp:100-103
        m.GetResult()
    assert e.value.code == 2
    aliased = list(win["bgrs"])
    aliased[1] = aliased[0]
    with pytest.raises(_lib.DrError) as e:  # dr_mvsnet.cpp:153-160
        m.CallAsync(64, 96, 3, win["ref_index"], aliased, win["K"], list(win["c2ws"]), 0.5, 5.0, 2.5)
    assert e.value.code == 1
    with pytest.raises(ValueError):  # images of another size than announced: caught by the Python mirror's size check
        m.CallAsync(60, 96, 3, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), 0.5, 5.0, 2.5)
    odd = [np.ascontiguousarray(b[:62]) for b in win["bgrs"]]
    with pytest.raises(_lib.DrError):  # a height the 3-stage pyramid cannot hold: rejected by the engine
        m.CallAsync(62, 96, 3, win["ref_index"], odd, win["K"], list(win["c2ws"]), 0.5, 5.0, 2.5)
    m.CallAsync(*args)  # still usable afterwards
    out = m.GetResult()
    assert np.isfinite(out.depth_dense).all()
    m.close()


def test_pipelined_calls_keep_order(trained_blob):
    """Back-to-back CallAsync/GetResult pairs on different windows (TandemBackend's usage, tandem_backend.cpp:147,268)."""
    from synth import scene
    from tandem_amd.dr_mvsnet import DrMvsnet
    m = DrMvsnet(trained_blob)
    wins = [scene.make_window(64, 96, 3, seed=s) for s in (1, 2, 1)]
    outs = []
    for w in wins:
        m.CallAsync(64, 96, 3, w["ref_index"], w["bgrs"], w["K"], list(w["c2ws"]), 0.5, 5.0, 2.5)
        outs.append(m.GetResult())
    assert np.array_equal(outs[0].depth_dense, outs[2].depth_dense)  # deterministic
    assert not np.array_equal(outs[0].depth_dense, outs[1].depth_dense)
    m.close()


def _edge_filter_is_exact(m, H, W):
    """Every discard percentage on one engine: the engine's edge measure, filtered depth and mask against the oracle filter on the engine's own depth."""
    import torch
    from oracle import mvsnet_oracle as O
    from synth import scene
    win = scene.make_window(H, W, 3, seed=4)
    for disc in (0.0, 2.5, 10.0, 37.5, 100.0):
        m.CallAsync(H, W, 3, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), 0.5, 5.0, disc)
        out = m.GetResult()
        filt, mask, edge, thr = O.filter_edges(torch.from_numpy(out.depth_dense.copy()), disc)
        assert np.array_equal(m.tensor("edge")[0, :, :, 0], edge.numpy()), disc
        assert np.array_equal(out.depth, filt.numpy()), disc
        assert np.array_equal(out.depth == 0, mask.numpy() | (out.depth_dense == 0)), disc
        print("edge filter %dx%d discard %5.1f: threshold %.6g, %d of %d pixels masked" % (H, W, disc, float(thr), int(mask.sum()), H * W))
        if disc == 0.0:  # the rank clamps to n - 1: the threshold is the maximum and nothing is masked
            assert float(thr) == float(edge.max()) and not mask.any() and np.array_equal(out.depth, out.depth_dense)
        if disc == 100.0:  # rank 0: the threshold is the minimum
            assert float(thr) == float(edge.min()) and np.array_equal(mask.numpy(), edge.numpy() > float(edge.min()))


@pytest.mark.parametrize("H,W", [(32, 32), (32, 96), (128, 160)], ids=["32x32", "32x96", "128x160"])
def test_edge_filter_is_exact_given_the_same_depth(trained_blob, H, W):
    """The order-statistic filter is pure comparisons: fed the engine's own depth map, the oracle filter must
    reproduce the engine's mask bit for bit (module.py:1320-1361).  Discard 0 and 100 are the two ends of the rank (n - 1 and 0); at 32 x 32 the select
    runs on n = 1024: four workgroups of the histogram kernels, mostly empty bins for the fused scans."""
    from tandem_amd.dr_mvsnet import DrMvsnet
    m = DrMvsnet(trained_blob)
    _edge_filter_is_exact(m, H, W)
    m.close()


@pytest.mark.parametrize("fused", ["0", "1"])
def test_edge_filter_is_exact_with_and_without_fused_scans(trained_blob, monkeypatch, parity_hooks, fused):
    """The same at 32 x 32 in both launch forms of the radix select (the parity build reads DR_FILTER_FUSED): a k_scan launch per level (8 launches) and
    the scans as the prologue of the kernels that follow them (5)."""
    from tandem_amd.dr_mvsnet import DrMvsnet
    monkeypatch.setenv("DR_FILTER_FUSED", fused)
    m = DrMvsnet(trained_blob)
    _edge_filter_is_exact(m, 32, 32)
    launches = [r["op"] for r in m.profile() if r["op"].startswith("filter.")]
    assert len(launches) == (5 if fused == "1" else 8), launches
    m.close()


def test_plain_variance_model_without_view_aggregation(tmp_path):
    """abl01/abl02 models: no gate, variance over all views incl. the reference (module.py:1074-1075,1094-1096,1110)."""
    from oracle import mvsnet_oracle as O
    from synth import scene
    from tandem_amd import weights as Wt
    from tandem_amd.dr_mvsnet import DrMvsnet
    tens = Wt.random_state((48, 32, 8), seed=11)
    blob = str(tmp_path / "nova.tdmw")
    Wt.write_blob(blob, tens, depth_num=(48, 32, 8), view_aggregation=False)
    meta, back = Wt.read_blob(blob)
    assert meta["view_aggregation"] is False
    win = scene.make_window(64, 96, 4, seed=8)
    ref = O.forward(O.Weights(meta, back), win["bgrs"], win["K"], win["c2ws"], win["ref_index"], 0.5, 5.0, 5.0)
    m = DrMvsnet(blob)
    m.CallAsync(64, 96, 4, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), 0.5, 5.0, 5.0)
    compare(m.GetResult(), ref, "no-VA")
    m.close()


def test_resolution_and_view_count_can_change_between_calls(trained_blob):
    """The engine re-plans when TANDEM changes the window shape (dr_mvsnet.cpp builds tensors per call)."""
    from oracle import mvsnet_oracle as O
    from synth import scene
    from tandem_amd import weights as Wt
    from tandem_amd.dr_mvsnet import DrMvsnet
    meta, tens = Wt.read_blob(trained_blob)
    w = O.Weights(meta, tens)
    m = DrMvsnet(trained_blob)
    for (H, W, V) in ((64, 96, 3), (96, 64, 5), (64, 96, 3), (128, 128, 2)):
        win = scene.make_window(H, W, V, seed=H + V)
        m.CallAsync(H, W, V, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), 0.5, 5.0, 2.5)
        out = m.GetResult()
        ref = O.forward(w, win["bgrs"], win["K"], win["c2ws"], win["ref_index"], 0.5, 5.0, 2.5)
        compare(out, ref, f"{H}x{W}x{V}")
    m.close()


def test_ref_index_and_view_order(trained_blob):
    """Model order is [ref, others in window order] (dr_mvsnet.cpp:190-197): permuting the window consistently with
    ref_index must not change the result when the source order is preserved."""
    from synth import scene
    from tandem_amd.dr_mvsnet import DrMvsnet
    win = scene.make_window(64, 96, 4, seed=6)  # ref_index = 2
    m = DrMvsnet(trained_blob)
    m.CallAsync(64, 96, 4, 2, win["bgrs"], win["K"], list(win["c2ws"]), 0.5, 5.0, 2.5)
    a = m.GetResult()
    order = [2, 0, 1, 3]  # same model order, reference now first
    m.CallAsync(64, 96, 4, 0, [win["bgrs"][i] for i in order], win["K"], [win["c2ws"][i] for i in order], 0.5, 5.0, 2.5)
    b = m.GetResult()
    assert np.array_equal(a.depth_dense, b.depth_dense) and np.array_equal(a.depth, b.depth)
    m.close()


def test_maximum_views_large_frame_and_textureless_input(trained_blob):
    """Edges of the supported range: view_num = 8 (kMaxSrc + 1), a 1280x960 frame (4x the headline size: every conv
    plan, halo tile and cost-volume grid is re-derived), and a textureless window (all views one grey level: the cost
    volume is exactly zero, every plane ties, depth = mean hypothesis) -- each against the oracle."""
    from oracle import mvsnet_oracle as O
    from synth import scene
    from tandem_amd import weights as Wt
    from tandem_amd.dr_mvsnet import DrMvsnet
    meta, tens = Wt.read_blob(trained_blob)
    w = O.Weights(meta, tens)
    m = DrMvsnet(trained_blob)
    win = scene.make_window(64, 96, 8, seed=8)
    m.CallAsync(64, 96, 8, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), 0.5, 5.0, 2.5)
    compare(m.GetResult(), O.forward(w, win["bgrs"], win["K"], win["c2ws"], win["ref_index"], 0.5, 5.0, 2.5), "v8")
    win = scene.make_window(960, 1280, 3, seed=9)
    m.CallAsync(960, 1280, 3, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), win["depth_min"], win["depth_max"], 10.0)
    compare(m.GetResult(), O.forward(w, win["bgrs"], win["K"], win["c2ws"], win["ref_index"], win["depth_min"], win["depth_max"], 10.0), "1280x960")
    win = scene.make_window(64, 96, 3, seed=1)
    grey = [np.full_like(b, 97) for b in win["bgrs"]]
    m.CallAsync(64, 96, 3, win["ref_index"], grey, win["K"], list(win["c2ws"]), 0.5, 5.0, 2.5)
    out = m.GetResult()
    ref = O.forward(w, grey, win["K"], win["c2ws"], win["ref_index"], 0.5, 5.0, 2.5)
    assert np.isfinite(out.depth_dense).all() and np.isfinite(out.confidence_dense).all()
    assert np.abs(out.depth_dense - ref["depth_dense"]).max() < 2e-3
    m.close()


def test_concurrent_engines_give_the_sequential_answer(trained_blob):
    """bench.py's throughput configuration: several DrMvsnet engines (own stream + worker each) running at once on
    one GPU must each return exactly what they return alone."""
    import threading
    from synth import scene
    from tandem_amd.dr_mvsnet import DrMvsnet
    wins = [scene.make_window(96, 128, 5, seed=20 + i) for i in range(3)]
    alone = []
    for win in wins:
        m = DrMvsnet(trained_blob)
        m.CallAsync(96, 128, 5, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), 0.5, 5.0, 5.0)
        alone.append(m.GetResult())
        m.close()
    engines = [DrMvsnet(trained_blob) for _ in wins]
    outs = [None] * len(wins)

    def work(i):
        for _ in range(4):
            win = wins[i]
            engines[i].CallAsync(96, 128, 5, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), 0.5, 5.0, 5.0)
            outs[i] = engines[i].GetResult()

    th = [threading.Thread(target=work, args=(i,)) for i in range(len(wins))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for a, b in zip(alone, outs):
        assert np.array_equal(a.depth_dense.view(np.uint32), b.depth_dense.view(np.uint32))
        assert np.array_equal(a.depth.view(np.uint32), b.depth.view(np.uint32))
        assert np.array_equal(a.confidence_dense.view(np.uint32), b.confidence_dense.view(np.uint32))
    for e in engines:
        e.close()


def test_autotuned_plan_stays_within_tolerance(trained_blob):
    """drm_autotune swaps convolution tilings by measured time; the result may move by accumulation order only."""
    from oracle import mvsnet_oracle as O
    from synth import scene
    from tandem_amd import weights as Wt
    from tandem_amd.dr_mvsnet import DrMvsnet
    meta, tens = Wt.read_blob(trained_blob)
    win = scene.make_window(96, 128, 5, seed=31)
    ref = O.forward(O.Weights(meta, tens), win["bgrs"], win["K"], win["c2ws"], win["ref_index"], 0.5, 5.0, 5.0)
    m = DrMvsnet(trained_blob)
    m.upload(96, 128, 5, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), 0.5, 5.0, 5.0)
    before, after = m.autotune(12)
    assert 0 < after <= before * 1.0001
    m.forward(1)
    compare(m.download(), ref, "autotuned")
    m.close()


def test_fused_skip_equals_the_two_kernel_path(trained_blob, monkeypatch, parity_hooks):
    """FeatureNet stage 3 (module.py:524-529): skip.stage3 + upsample computed inside out.stage3's staging step gives
    bit-for-bit what k_skip_up followed by the plain convolution gives (a second shape with partial tiles)."""
    from synth import scene
    from tandem_amd.dr_mvsnet import DrMvsnet
    monkeypatch.setenv("DR_OUT3_FOLDED", "0")  # (the default since round 3 is the folded form, tested below)
    outs = []
    for unfused in (False, True):
        if unfused:
            monkeypatch.setenv("DR_NO_SKIP_FUSION", "1")
        m = DrMvsnet(trained_blob)
        res = []
        for (h, w, v) in ((64, 96, 3), (96, 160, 4)):
            win = scene.make_window(h, w, v, seed=5)
            m.CallAsync(h, w, v, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), 0.5, 5.0, 2.5)
            res.append(m.GetResult())
        outs.append(res)
        m.close()
    for a, b in zip(*outs):
        assert np.array_equal(a.depth_dense, b.depth_dense) and np.array_equal(a.confidence_dense, b.confidence_dense)
        assert np.array_equal(a.depth, b.depth) and np.array_equal(a.confidence, b.confidence)


def test_fused_front_equals_the_three_kernel_path(trained_blob, monkeypatch, parity_hooks):
    """FeatureNet's first block (module.py:461-470; u8 -> float as dr_mvsnet.cpp:184-217) in one launch (k_fn_front, csrc/fn_front.h: the
    float image and conv0.0's output never leave the CU) against k_preprocess + the two convolution launches in their direct form: the same
    products in the same order, so `fn.conv0.1` agrees bit for bit wherever the direct plan keeps one accumulator per position tile (every
    instance except the narrow K loop's CT * PT = 1, which adds two partial sums: fp32 reassociation there).  Widths that are not a multiple
    of the kernel's 64-pixel tile included."""
    import re
    from synth import scene
    from tandem_amd.dr_mvsnet import DrMvsnet
    shapes = ((64, 96, 3), (96, 160, 4), (224, 352, 3))
    runs = []
    for env in ({}, {"DR_FN_FRONT": "0", "DR_CONV_WINO": "0", "DR_CONV_NO_TUNED": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m = DrMvsnet(trained_blob)
        res = []
        for (h, w, v) in shapes:
            win = scene.make_window(h, w, v, seed=11)
            m.upload(h, w, v, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), 0.5, 5.0, 2.5)
            m.forward(1)
            prof = {r["op"]: r["kernel"] for r in m.profile()}
            res.append((m.tensor("fn.conv0.1").copy(), prof))
        runs.append(res)
        m.close()
        for k in env:
            monkeypatch.delenv(k)
    for (fa, pa), (fb, pb) in zip(*runs):
        assert pa.get("fn.front") == "k_fn_front" and "fn.conv0.0" not in pa, pa
        assert "fn.front" not in pb and "preprocess" in pb and pb["fn.conv0.1"].startswith("k_conv"), pb
        assert fa.shape == fb.shape and np.isfinite(fa).all() and np.abs(fb).max() > 0.1
        single_chain = all(int(re.findall(r"\d+", pb[n])[2]) >= 2 for n in ("fn.conv0.0", "fn.conv0.1"))
        if single_chain:
            assert np.array_equal(fa, fb), (pb["fn.conv0.0"], pb["fn.conv0.1"], np.abs(fa - fb).max())
        else:
            assert np.abs(fa - fb).max() <= 2e-6 * np.abs(fb).max(), (pb["fn.conv0.0"], pb["fn.conv0.1"], np.abs(fa - fb).max())


def test_fused_head3_equals_the_four_launch_form(trained_blob, monkeypatch, parity_hooks):
    """FeatureNet's folded stage-3 head (module.py:480-485,524-529) in one launch (k_fn_head3, csrc/fn_head3.h: conv3x3(conv0; Wout . Wskip),
    the two row-parity phase layers over inter2 and the border term meet in one accumulator) against the four launches fn.out3a..d: the
    same three terms, their partial sums added in another order (and fn.out3a in the Winograd form there) -- fp32 reassociation, held to
    5e-6 of feat3's range; the zero border of the padded tensor stays untouched.  Widths that are not a multiple of the 64-pixel tile included."""
    from synth import scene
    from tandem_amd.dr_mvsnet import DrMvsnet
    shapes = ((64, 96, 3), (96, 160, 4), (224, 352, 3))
    runs = []
    for env in ({}, {"DR_FN_HEAD3": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m = DrMvsnet(trained_blob)
        res = []
        for (h, w, v) in shapes:
            win = scene.make_window(h, w, v, seed=12)
            m.upload(h, w, v, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), 0.5, 5.0, 2.5)
            m.forward(1)
            prof = {r["op"]: r["kernel"] for r in m.profile()}
            res.append((m.tensor("feat3").copy(), prof, m.download().depth_dense.copy()))
        runs.append(res)
        m.close()
        for k in env:
            monkeypatch.delenv(k)
    for (fa, pa, da), (fb, pb, db) in zip(*runs):
        assert pa.get("fn.head3") == "k_fn_head3" and "fn.out3a" not in pa, pa
        assert "fn.head3" not in pb and all(n in pb for n in ("fn.out3a", "fn.out3b", "fn.out3c", "fn.out3d")), pb
        assert fa.shape == fb.shape and np.isfinite(fa).all() and np.abs(fb).max() > 0.1
        assert np.abs(fa - fb).max() <= 5e-6 * np.abs(fb).max(), np.abs(fa - fb).max() / np.abs(fb).max()
        assert np.abs(da - db).mean() < 1e-4


def test_fewer_launches_at_the_tail_are_bit_identical(trained_blob, tmp_path, monkeypatch, parity_hooks):
    """Round 5's two launch reductions behind the last convolution, each against the form it replaces, bit for bit on every output:
    (1) the edge filter's radix select with every level's scan as the prologue of the kernel that follows it (k_hist_s / k_apply_s, 8 -> 5
    launches; module.py:1320-1361) -- integers only; (2) softmax / expectation / confidence in the launch that computes the logits where a
    stage's planes are one depth chunk (k_prob2_regress, D = 8; module.py:1116-1133) -- the same expressions on the same values."""
    from synth import scene
    from tandem_amd import weights as Wt
    from tandem_amd.dr_mvsnet import DrMvsnet
    _, tens = Wt.read_blob(trained_blob)
    blobs = [trained_blob]
    p = str(tmp_path / "w_48_8_8.tdmw")  # a second plane configuration: two stages with D = 8
    Wt.write_blob(p, Wt.random_state((48, 8, 8), seed=3), depth_num=(48, 8, 8), view_aggregation=True)
    blobs.append(p)
    monkeypatch.setenv("DR_PROB_ZCHUNK", "8")  # (small frames: keep a D = 8 stage in one depth chunk, as the full-size frame has it by itself)
    for blob in blobs:
        runs = []
        for env in ({}, {"DR_FILTER_FUSED": "0"}, {"DR_PROB_REGRESS": "0"}):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            m = DrMvsnet(blob)
            res = []
            for (h, w, v, disc) in ((64, 96, 3, 2.5), (96, 160, 4, 10.0), (224, 352, 3, 0.0)):
                win = scene.make_window(h, w, v, seed=13)
                m.upload(h, w, v, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), 0.5, 5.0, disc)
                m.forward(1)
                prof = {r["op"]: r["kernel"] for r in m.profile()}
                out = m.download()
                res.append((prof, m.tensor("edge").copy(), out.depth.copy(), out.confidence.copy(), out.depth_dense.copy(), out.confidence_dense.copy(),
                            m.tensor("depth2").copy(), m.tensor("conf2").copy()))
            runs.append(res)
            m.close()
            for k in env:
                monkeypatch.delenv(k)
        for a, b, c in zip(*runs):
            assert "filter.scan0" not in a[0] and "filter.scan0" in b[0] and "filter.scan2" in b[0], (a[0], b[0])
            assert a[0]["s3.prob"] == "k_prob2_regress<8>" and c[0]["s3.prob"] == "k_prob2<1>", (a[0]["s3.prob"], c[0]["s3.prob"])
            if blob != trained_blob:
                assert a[0]["s2.prob"] == "k_prob2_regress<8>" and a[0]["s1.prob"] == "k_prob2<1>"
            for other in (b, c):
                for x, y in zip(a[1:], other[1:]):
                    assert np.array_equal(x, y)
            assert np.isfinite(a[4]).all()


def test_fused_skip_on_the_marching_kernel(trained_blob, monkeypatch, parity_hooks):
    """out.stage3 with the skip computed by k_conv_m's producer waves (conv_march.h, march_producer_fz) against the same
    layer on k_conv's fused staging: same fmaf chain in the skip, same channel-pass and tap order in the 3x3 layer, so
    feat3 agrees to fp32 reassociation at most (tolerance 2e-5 of the tensor's range; observed: bit-identical)."""
    from synth import scene
    from tandem_amd.dr_mvsnet import DrMvsnet
    monkeypatch.setenv("DR_OUT3_FOLDED", "0")
    feats = []
    for env in ({"DR_CONV_MARCH": "2", "DR_CONV_NO_TUNED": "1"}, {"DR_FZ_NO_MARCH": "1", "DR_CONV_NO_TUNED": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m = DrMvsnet(trained_blob)
        res = []
        for (h, w, v) in ((96, 160, 4), (224, 352, 3)):
            win = scene.make_window(h, w, v, seed=6)
            m.upload(h, w, v, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), 0.5, 5.0, 2.5)
            m.forward(1)
            prof = {r["op"]: r["kernel"] for r in m.profile()}
            res.append((m.tensor("feat3").copy(), prof["fn.out3"]))
        feats.append(res)
        m.close()
        for k in env:
            monkeypatch.delenv(k)
    for (fa, ka), (fb, kb) in zip(*feats):
        assert "k_conv_m" in ka and "k_conv_m" not in kb, (ka, kb)
        assert np.abs(fa - fb).max() <= 2e-5 * np.abs(fb).max()


def test_register_regression_equals_the_three_pass_kernel(trained_blob, tmp_path, monkeypatch, parity_hooks):
    """Round 3's k_regress_r<D> (the pixel's logits in registers, one round of loads) against the three-pass k_regress: same
    expressions in the same order -- at plane counts with a register instance (48/32/8, 48/4/4) and without (16/8/8: the generic
    kernel either way): all four output maps equal bit for bit (both kernels take the exponential through expf_value(), which
    keeps hipcc from fusing its last multiply into one spelling's sum and not the other's)."""
    from synth import scene
    from tandem_amd import weights as Wt
    from tandem_amd.dr_mvsnet import DrMvsnet
    _, tens = Wt.read_blob(trained_blob)
    blobs = [trained_blob]
    for planes in ((48, 4, 4), (16, 8, 8)):
        b = str(tmp_path / ("w_%d_%d_%d.tdmw" % planes))
        Wt.write_blob(b, tens, depth_num=planes)
        blobs.append(b)
    for blob in blobs:
        outs = []
        for old in (False, True):
            if old:
                monkeypatch.setenv("DR_REGRESS_GENERIC", "1")
            m = DrMvsnet(blob)
            res = []
            for rep, (h, w, v) in enumerate(((96, 160, 4), (128, 224, 3))):
                win = scene.make_window(h, w, v, seed=7 + rep)
                m.CallAsync(h, w, v, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), 0.5, 5.0, 10.0)
                res.append(m.GetResult())
            outs.append(res)
            m.close()
            if old:
                monkeypatch.delenv("DR_REGRESS_GENERIC")
        for a, b in zip(*outs):
            dd = np.abs(a.depth_dense - b.depth_dense) / np.maximum(np.abs(b.depth_dense), 1e-3)
            dc = np.abs(a.confidence_dense - b.confidence_dense)
            print("regress A/B:", os.path.basename(blob), "max rel depth diff %.3e, conf diff > 1e-5 at %.2e of pixels, max %.3e" % (dd.max(), (dc > 1e-5).mean(), dc.max()))
            assert np.array_equal(a.depth_dense, b.depth_dense) and np.array_equal(a.confidence_dense, b.confidence_dense)
            assert np.array_equal(a.depth, b.depth) and np.array_equal(a.confidence, b.confidence)


def test_folded_out_stage3_equals_the_literal_order(trained_blob, monkeypatch, parity_hooks):
    """Round 3's default for FeatureNet's stage-3 head: out.stage3(up(inter2) + skip.stage3(c3)) evaluated as conv3x3(c3; Wout.Wskip)
    + conv3x3 over the upsampled inter2 at half resolution (ConvLayer::up2) + a border-corrected bias, against the fused-skip form
    that follows the reference's order (module.py:524-529).  Linear algebra only, so feat3 agrees to fp32 reassociation:
    2e-5 of its range, everywhere incl. the image border and partial tiles; the depth maps agree within the pipeline's tolerance."""
    from synth import scene
    from tandem_amd.dr_mvsnet import DrMvsnet
    res = []
    for folded, head3 in (("1", "1"), ("1", "0"), ("0", "1")):  # the folded form in one launch (k_fn_head3, the default since round 5) and in four; the literal order
        monkeypatch.setenv("DR_OUT3_FOLDED", folded)
        monkeypatch.setenv("DR_FN_HEAD3", head3)
        m = DrMvsnet(trained_blob)
        out = []
        for (h, w, v) in ((96, 160, 4), (224, 352, 3), (64, 96, 2)):
            win = scene.make_window(h, w, v, seed=6)
            m.upload(h, w, v, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), 0.5, 5.0, 2.5)
            m.forward(1)
            ops = [r["op"] for r in m.profile()]
            out.append((m.tensor("feat3").copy(), m.download().depth_dense.copy(), ops))
        res.append(out)
        m.close()
    for (f1, d1, o1), (f4, d4, o4), (fb, db, ob) in zip(*res):
        assert "fn.head3" in o1 and "fn.out3a" not in o1, o1
        assert "fn.out3a" in o4 and "fn.out3d" in o4 and "fn.out3" in ob and "fn.head3" not in ob, (o4, ob)
        scale = np.abs(fb).max()
        for fa, da in ((f1, d1), (f4, d4)):
            assert np.abs(fa - fb).max() <= 2e-5 * scale, np.abs(fa - fb).max() / scale
            for sl in (np.s_[:, 0], np.s_[:, -1], np.s_[:, :, 0], np.s_[:, :, -1]):  # the four image borders
                assert np.abs(fa[sl] - fb[sl]).max() <= 2e-5 * scale
            assert np.abs(da - db).mean() < 1e-4 and np.abs(da - db).max() < 5e-2


@pytest.mark.parametrize("views", [2, 3, 4, 6, 7])
def test_shared_setup_cost_volume_is_bit_identical(trained_blob, tmp_path, monkeypatch, views, parity_hooks):
    """k_costvol3 (the lanes of a pixel take different (plane, view) samples of a batch, set them up once and hand the tap offset
    and weights round by DPP) against k_costvol2 (every lane sets up every sample): same products in the same order, so the
    three cost volumes are equal bit for bit -- 1 to 6 source views (batches that straddle planes), view aggregation and plain
    variance, two shapes (partial pixel blocks)."""
    from synth import scene
    from tandem_amd import weights as Wt
    from tandem_amd.dr_mvsnet import DrMvsnet
    meta, tens = Wt.read_blob(trained_blob)
    plain = str(tmp_path / "plain.tdmw")
    Wt.write_blob(plain, {k: v for k, v in tens.items() if not k.startswith("volume_gates.")}, depth_num=(16, 8, 4), view_aggregation=False)
    for blob in (trained_blob, plain):
        vols = []
        for old in (False, True):
            if old:
                monkeypatch.setenv("DR_COSTVOL_V2", "1")
            m = DrMvsnet(blob)
            res = []
            for (h, w) in ((96, 160), (64, 224)):
                win = scene.make_window(h, w, views, seed=11)
                m.upload(h, w, views, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), 0.5, 5.0, 2.5)
                m.forward(1)
                kern = {r["op"]: r["kernel"] for r in m.profile()}
                res.append(([m.tensor("volume%d" % s).copy() for s in (1, 2, 3)], kern["s2.costvol"]))
            vols.append(res)
            m.close()
            if old:
                monkeypatch.delenv("DR_COSTVOL_V2")
        for (va, ka), (vb, kb) in zip(*vols):
            # (since round 6 the view-aggregation model's volumes come from k_costvol5, the plain-variance model's still from k_costvol3)
            assert ka.startswith("k_costvol5" if blob == trained_blob else "k_costvol3") and kb.startswith("k_costvol2"), (ka, kb)
            for a, b in zip(va, vb):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), np.abs(a - b).max()


@pytest.mark.parametrize("views,dmin,dmax", [(7, 0.5, 5.0), (7, 0.01, 10.0), (3, 0.5, 5.0), (2, 0.3, 1.2), (5, 2.0, 40.0), (8, 0.5, 5.0)])
def test_view_outer_cost_volume_is_bit_identical(trained_blob, monkeypatch, views, dmin, dmax, parity_hooks):
    """k_costvol5 (round 6: view outer, the planes of a depth chunk inner, one float4 accumulator per plane in registers, the view's matrix
    in scalar registers, the pixel's ray hoisted out of the plane loop) against k_costvol3 (plane outer, view inner, one accumulator):
    per voxel the views are added in the same order with the same products, so the three cost volumes -- and everything behind them --
    are equal bit for bit.  Depth ranges as in the LDS-staged kernel's test (samples outside every view, sub-pixel steps; at 0.01 .. 10 about
    1 % of the samples of stages 1 and 2 lie behind a source camera, but with the scene's poses every one of them falls outside the source image
    as well, so the pz < 0.001 mask itself decides nothing in these windows -- tests/test_mvs_stage_ref.py shows it, tests/test_mvs_stages_gpu.py
    has the windows where it does); 1 to 7 source views; depth chunks of 4 planes (the product's choice) and of 8 (DR_CV_DCHUNK*); and the kernel's two A/B forms of
    the parity build: every sample gathering its taps (DR_CV5_REUSE=0: the product skips a sample's gathers where its footprint is the
    previous plane's and copies the taps), one-row and four-row workgroup tiles at every stage (DR_CV5_ROWS)."""
    from synth import scene
    from tandem_amd.dr_mvsnet import DrMvsnet
    variants = [(None, {}), ("8", {})]
    if views in (7, 3):
        variants += [(None, {"DR_CV5_REUSE": "0"}), (None, {"DR_CV5_ROWS": "1"}), ("8", {"DR_CV5_ROWS": "4"})]
    for dch, extra in variants:
        for s in (1, 2, 3):
            if dch:
                monkeypatch.setenv("DR_CV_DCHUNK%d" % s, dch)
            else:
                monkeypatch.delenv("DR_CV_DCHUNK%d" % s, raising=False)
        vols = []
        for old in (False, True):
            for k in ("DR_CV5_REUSE", "DR_CV5_ROWS"):
                monkeypatch.delenv(k, raising=False)
            if old:
                monkeypatch.setenv("DR_COSTVOL_V3", "1")
            else:
                monkeypatch.delenv("DR_COSTVOL_V3", raising=False)
                for k, v in extra.items():
                    monkeypatch.setenv(k, v)
            m = DrMvsnet(trained_blob)
            res = []
            for (h, w) in ((96, 160), (64, 224), (256, 320)):
                win = scene.make_window(h, w, views, seed=17)
                m.upload(h, w, views, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), dmin, dmax, 2.5)
                m.forward(1)
                kern = {r["op"]: r["kernel"] for r in m.profile()}
                res.append(([m.tensor("volume%d" % s).copy() for s in (1, 2, 3)], [kern["s%d.costvol" % s] for s in (1, 2, 3)], m.download().depth_dense.copy()))
            vols.append(res)
            m.close()
        for k in ("DR_COSTVOL_V3", "DR_CV5_REUSE", "DR_CV5_ROWS"):
            monkeypatch.delenv(k, raising=False)
        for (va, ka, da), (vb, kb, db) in zip(*vols):
            assert all(k.startswith("k_costvol5") for k in ka) and all(k.startswith("k_costvol3") for k in kb), (ka, kb)
            assert all(k.endswith(",%s>" % (dch or "4")) for k in ka), ka
            for a, b in zip(va, vb):
                assert np.isfinite(a).all()
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (np.abs(a - b).max(), (a != b).mean())
            assert np.array_equal(da.view(np.uint32), db.view(np.uint32))


@pytest.mark.parametrize("views,dmin,dmax", [(7, 0.5, 5.0), (7, 0.01, 10.0), (3, 0.5, 5.0), (2, 0.3, 1.2), (5, 2.0, 40.0)])
def test_lds_staged_cost_volume_is_bit_identical(trained_blob, monkeypatch, views, dmin, dmax, parity_hooks):
    """k_costvol4 (round 4: the taps of a pixel tile's samples staged once per (view, 4 planes) step into LDS by LDS-DMA, read from there)
    against k_costvol3 (every tap a gather from global memory): the same arithmetic on the same tap values in the same view order, so the
    three cost volumes are equal bit for bit.  The depth ranges make the kernel take every path: boxes that fit (the scene's own range),
    steps whose planes lie metres apart or in front of the cameras so that the box does not fit or no sample falls inside the view
    (0.01 .. 10 as the headline runs it, 2 .. 40; the samples that 0.01 .. 10 puts behind a source camera are all outside its image too: the
    behind-camera mask is not what these windows exercise, see tests/test_mvs_stage_ref.py), a narrow range (sub-pixel steps), 1 to 6 source views, two shapes."""
    from synth import scene
    from tandem_amd.dr_mvsnet import DrMvsnet
    vols = []
    for old in (False, True):
        monkeypatch.setenv("DR_CV4_STAGES", "0" if old else "7")  # (k_costvol4 lives in the parity build: measured slower than k_costvol3)
        if old:
            monkeypatch.setenv("DR_COSTVOL_V3", "1")                # (the product's own sweep is k_costvol5 since round 6: compare with the kernel k_costvol4 was derived from)
        else:
            monkeypatch.delenv("DR_COSTVOL_V3", raising=False)
        monkeypatch.setenv("DR_CV4_SP8", "0" if views == 3 else "6")
        m = DrMvsnet(trained_blob)
        res = []
        for (h, w) in ((96, 160), (64, 224), (256, 320)):
            win = scene.make_window(h, w, views, seed=13)
            m.upload(h, w, views, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), dmin, dmax, 2.5)
            m.forward(1)
            kern = {r["op"]: r["kernel"] for r in m.profile()}
            res.append(([m.tensor("volume%d" % s).copy() for s in (1, 2, 3)], [kern["s%d.costvol" % s] for s in (1, 2, 3)], m.download().depth_dense.copy()))
        vols.append(res)
        m.close()
    monkeypatch.delenv("DR_COSTVOL_V3", raising=False)
    for (va, ka, da), (vb, kb, db) in zip(*vols):
        assert all(k.startswith("k_costvol4") for k in ka) and all(k.startswith("k_costvol3") for k in kb), (ka, kb)
        for a, b in zip(va, vb):
            assert np.isfinite(a).all()
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (np.abs(a - b).max(), (a != b).mean())
        assert np.array_equal(da.view(np.uint32), db.view(np.uint32))


# ---- the opt-in bf16 x 3 precision mode (csrc/conv_bf3.h, DR_CONV_BF16X3=1; first run on a GPU in round 4: green) ----
@pytest.mark.parametrize("path", [p for p in GOLD if "rand" not in p and "novar" not in p], ids=lambda p: os.path.basename(p))
def test_bf16x3_mode_stays_inside_the_fp32_bounds(path, trained_blob, tmp_path, monkeypatch, parity_hooks):
    """With every convolution (Cin % 8 == 0) on k_conv_b the depth maps must still pass the bounds the fp32 path is held to -- what
    tools/study_split_bf16.py predicts from the oracle (mean 2e-5 m, max 2e-4 m) -- and must differ from the fp32 engine's.
    Run with strictly sequential kernels (DR_MVS_NO_SIDE_STREAM): round 6 found that this parity-build-only mode is NOT bit-stable from run to run
    when its unfused FeatureNet head launches overlap the stage-1 plane sweep (tools/study/determinism.py: the stage-1 volume differs in ~50 voxels per
    run, enough to move one pixel by 5-10 mm and trip the pairwise bound below); sequentially it is, and the fp32 product path is bit-stable either way
    (16 of 16 runs, same script).  The mode left the product library in round 6; the interaction was not pursued."""
    from tandem_amd.dr_mvsnet import DrMvsnet
    monkeypatch.setenv("DR_MVS_NO_SIDE_STREAM", "1")
    g = np.load(path)
    blob = blob_for(g, trained_blob, tmp_path)
    bgrs = [np.ascontiguousarray(b) for b in g["bgrs"]]
    H, W = bgrs[0].shape[:2]
    args = (H, W, len(bgrs), int(g["ref_index"]), bgrs, g["K"], list(g["c2ws"]), float(g["depth_min"]), float(g["depth_max"]), float(g["discard"]))
    outs = []
    for mode in ("1", None):
        if mode:
            monkeypatch.setenv("DR_CONV_BF16X3", mode)
        else:
            monkeypatch.delenv("DR_CONV_BF16X3", raising=False)
        m = DrMvsnet(blob)
        m.CallAsync(*args)
        outs.append(m.GetResult())
        m.close()
    ref = {k: g[f"ref_s3_{k}"] for k in ("depth", "confidence", "depth_dense", "confidence_dense")}
    compare(outs[0], ref, "bf16x3 " + os.path.basename(path), max_err=5e-2)  # 16-bit operands: the opt-in mode keeps round 4's single-pixel bound
    assert not np.array_equal(outs[0].depth_dense, outs[1].depth_dense)  # the mode really ran
    # (2e-3 m at the scene's 4.5 m depth range; the bound scales with the range, i.e. with the spacing of the hypothesis planes)
    assert np.abs(outs[0].depth_dense - outs[1].depth_dense).max() < 4.5e-4 * (float(g["depth_max"]) - float(g["depth_min"]))


# ---- the Winograd F(2,3) form of the stride-1 3-tap layers (csrc/conv_wino.h) ----
@pytest.mark.parametrize("path", [p for p in GOLD if "novar" not in p], ids=lambda p: os.path.basename(p))
def test_winograd_form_stays_inside_the_fp32_bounds(path, trained_blob, tmp_path, monkeypatch):
    """DR_CONV_WINO=2 puts every layer the form applies to (3-tap stride-1 y axis, even output height) on k_conv_w -- far more layers than
    the tuned plan table does by default -- and the depth maps must still pass the bounds of the direct kernels against the reference's
    outputs: the transform is fp32-exact algebra, it may only reassociate.  The engines must differ (the form really ran) and agree to
    the level the autotuned-plan test allows for any re-tiling."""
    from tandem_amd.dr_mvsnet import DrMvsnet
    g = np.load(path)
    blob = blob_for(g, trained_blob, tmp_path)
    bgrs = [np.ascontiguousarray(b) for b in g["bgrs"]]
    H, W = bgrs[0].shape[:2]
    args = (H, W, len(bgrs), int(g["ref_index"]), bgrs, g["K"], list(g["c2ws"]), float(g["depth_min"]), float(g["depth_max"]), float(g["discard"]))
    outs = []
    for mode in ("2", "0"):
        monkeypatch.setenv("DR_CONV_WINO", mode)
        m = DrMvsnet(blob)
        m.CallAsync(*args)
        outs.append(m.GetResult())
        m.close()
    ref = {k: g[f"ref_s3_{k}"] for k in ("depth", "confidence", "depth_dense", "confidence_dense")}
    compare(outs[0], ref, "winograd " + os.path.basename(path))
    compare(outs[1], ref, "direct " + os.path.basename(path))
    assert not np.array_equal(outs[0].depth_dense, outs[1].depth_dense)
    d = np.abs(outs[0].depth_dense - outs[1].depth_dense)
    assert d.mean() < 2e-5 * (float(g["depth_max"]) - float(g["depth_min"])), d.mean()


def test_pinned_upload_and_result_view_equal_the_copying_boundary(trained_blob):
    """The boundary extensions (include/dr_mi355x.h: drm_host_alloc, drm_get_result_view): a window whose images live in page-locked memory
    is uploaded in place -- and may be overwritten as soon as CallAsync returns -- and the result comes back as views of the engine's two
    alternating pinned blocks: bit-identical maps, a view survives exactly one further call."""
    from synth import scene
    from tandem_amd.dr_mvsnet import DrMvsnet
    H, W, V = 128, 160, 4
    w = scene.make_window(H, W, V, seed=3)
    args = lambda imgs: (H, W, V, w["ref_index"], imgs, w["K"], list(w["c2ws"]), w["depth_min"], w["depth_max"], 10.0)
    m = DrMvsnet(trained_blob)
    m.CallAsync(*args(w["bgrs"]))
    ref = m.GetResult()
    pinned = m.alloc_images(V, H, W)
    for p, b in zip(pinned, w["bgrs"]):
        p[...] = b
    m.CallAsync(*args(pinned))
    for p in pinned:
        p[...] = 0  # the upload has completed: the caller's buffers are its own again
    v1 = m.GetResultView()
    for k in ("depth", "confidence", "depth_dense", "confidence_dense"):
        assert np.array_equal(getattr(v1, k), getattr(ref, k)), k
    with pytest.raises(Exception):
        m.GetResultView()  # one result per call, as GetResult
    w2 = scene.make_window(H, W, V, seed=4)
    m.CallAsync(H, W, V, w2["ref_index"], w2["bgrs"], w2["K"], list(w2["c2ws"]), w2["depth_min"], w2["depth_max"], 10.0)
    v2 = m.GetResultView()
    assert np.array_equal(v1.depth_dense, ref.depth_dense)      # the first view is still intact after one further call ...
    assert not np.array_equal(v2.depth_dense, ref.depth_dense)  # ... which went to the other block
    mixed = [pinned[0]] + list(w["bgrs"][1:])                   # one pageable image: the staging path, same answer
    pinned[0][...] = w["bgrs"][0]
    m.CallAsync(*args(mixed))
    v3 = m.GetResult()
    assert np.array_equal(v3.depth_dense, ref.depth_dense)
    m.close()


# ---- the key-frame feature cache (round 6; drm_set_feature_cache) ----
def _sliding_windows(h, w, n_windows, seed):
    """A synthetic sliding key-frame sequence: 7 + n_windows - 1 images of one scene with their poses; window k = images k .. k + 6 (six of them were
    in window k - 1), reference = the second newest, as TANDEM builds it (FullSystem.cpp:1127)."""
    from synth import scene
    big = scene.make_window(h, w, 7 + n_windows - 1, seed=seed)
    for k in range(n_windows):
        yield dict(bgrs=[np.ascontiguousarray(b) for b in big["bgrs"][k:k + 7]], c2ws=list(big["c2ws"][k:k + 7]), K=big["K"], ref_index=5)


@pytest.mark.parametrize("h,w", [(96, 160), (224, 352)])
def test_feature_cache_is_bit_identical(trained_blob, h, w):
    """Cache on against cache off over a sliding sequence: every window's four maps are equal bit for bit (the single-view FeatureNet plan is built
    from the batch plan's own kernel instances); the first window takes the batch path and fills the cache, every later window computes ONE view;
    a change of resolution evicts everything and the cache works again at the new shape."""
    from tandem_amd.dr_mvsnet import DrMvsnet
    a, b = DrMvsnet(trained_blob), DrMvsnet(trained_blob)
    b.set_feature_cache(12)
    n = 5
    for shape in ((h, w), (64, 96), (h, w)):
        before = b.feature_cache_stats()
        for k, win in enumerate(_sliding_windows(shape[0], shape[1], n, seed=31)):
            outs = []
            for m in (a, b):
                m.CallAsync(shape[0], shape[1], 7, win["ref_index"], win["bgrs"], win["K"], win["c2ws"], 0.5, 5.0, 10.0)
                outs.append(m.GetResult())
            for name in ("depth", "confidence", "depth_dense", "confidence_dense"):
                x, y = getattr(outs[0], name), getattr(outs[1], name)
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (shape, k, name, np.abs(x - y).max())
        st = b.feature_cache_stats()
        assert st["single_view_plan"] and st["key_collisions"] == 0
        assert st["batch_windows"] - before["batch_windows"] == 1, st                      # the first window of a shape
        assert st["views_from_cache"] - before["views_from_cache"] == 6 * (n - 1), st      # six hits in each of the others
        assert st["views_computed"] - before["views_computed"] == 7 + (n - 1), st
    assert a.feature_cache_stats()["views_from_cache"] == 0
    a.close(); b.close()


def test_feature_cache_catches_a_key_collision(trained_blob):
    """The cache's key samples the image (first / last 64 bytes + 512 evenly spaced words); a hit is made exact by the device compare.  An image that
    differs from a cached one ONLY in bytes the key does not sample finds that entry -- the compare must notice, and the window's result must be the
    one of an engine without a cache."""
    from tandem_amd.dr_mvsnet import DrMvsnet
    h, w = 96, 160
    wins = list(_sliding_windows(h, w, 2, seed=33))
    a, b = DrMvsnet(trained_blob), DrMvsnet(trained_blob)
    b.set_feature_cache(10)
    args = lambda win: (h, w, 7, win["ref_index"], win["bgrs"], win["K"], win["c2ws"], 0.5, 5.0, 10.0)  # noqa: E731
    b.CallAsync(*args(wins[0])); b.GetResult()
    win = dict(wins[1])
    forged = [x.copy() for x in win["bgrs"]]
    n = h * w * 3
    step = (n // 512) & ~7
    flat = forged[2].reshape(-1)
    assert step >= 40
    flat[200 * step + 16: 200 * step + 32] ^= 0x5A  # between two sampled words (200 * step and 201 * step), away from the first and last 64 bytes
    win["bgrs"] = forged
    outs = []
    for m in (a, b):
        m.CallAsync(*args(win))
        outs.append(m.GetResult())
    st = b.feature_cache_stats()
    assert st["key_collisions"] == 1, st
    for name in ("depth", "confidence", "depth_dense", "confidence_dense"):
        assert np.array_equal(getattr(outs[0], name).view(np.uint32), getattr(outs[1], name).view(np.uint32)), name
    # ... and the engine goes on: the next window is computed as a batch and fills the cache again
    b.CallAsync(*args(wins[1])); r = b.GetResult()
    a.CallAsync(*args(wins[1])); r0 = a.GetResult()
    assert np.array_equal(r.depth_dense.view(np.uint32), r0.depth_dense.view(np.uint32))
    a.close(); b.close()


def test_engines_in_flight_are_bit_stable(trained_blob):
    """bench.py's configuration -- several DrMvsnet engines driven from as many threads -- must give every engine the single-engine result bit for bit: the
    engines share nothing but the device (round 6, after the parity-only bf16x3 mode turned out not to be run-to-run stable beside concurrent launches)."""
    import threading
    from synth import scene
    from tandem_amd.dr_mvsnet import DrMvsnet
    h, w = 224, 352
    win = scene.make_window(h, w, 7, seed=41)
    args = (h, w, 7, win["ref_index"], win["bgrs"], win["K"], list(win["c2ws"]), 0.01, 10.0, 10.0)
    ref = DrMvsnet(trained_blob)
    ref.upload(*args); ref.forward(1)
    names = ("volume1", "volume2", "volume3", "depth3", "conf3")
    want = {n: ref.tensor(n).copy() for n in names}
    engines = [DrMvsnet(trained_blob) for _ in range(4)]
    for m in engines:
        m.upload(*args)
    for _ in range(3):
        th = [threading.Thread(target=lambda m=m: m.forward(4)) for m in engines]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for m in engines:
            for n in names:
                assert np.array_equal(m.tensor(n).view(np.uint32), want[n].view(np.uint32)), n
    for m in engines + [ref]:
        m.close()


def test_feature_cache_with_page_locked_images(trained_blob):
    """The cache's CallAsync path (the new image uploaded first, the forward enqueued by the calling thread while the helper thread uploads the cached images on a second
    stream, their comparison last) with images in page-locked memory, which are uploaded IN PLACE: same maps as an engine without the cache, and the images may
    be overwritten as soon as CallAsync has returned."""
    from synth import scene
    from tandem_amd.dr_mvsnet import DrMvsnet
    h, w, n = 96, 160, 5
    big = scene.make_window(h, w, 7 + n - 1, seed=35)
    a, b = DrMvsnet(trained_blob), DrMvsnet(trained_blob)
    b.set_feature_cache(12)
    pinned = b.alloc_images(7, h, w)  # ONE set of page-locked buffers, refilled for every window (what a caller that reuses its buffers does)
    for k in range(n):
        imgs = [np.ascontiguousarray(x) for x in big["bgrs"][k:k + 7]]
        for dst, src in zip(pinned, imgs):
            dst[...] = src
        c2ws = list(big["c2ws"][k:k + 7])
        b.CallAsync(h, w, 7, 5, pinned, big["K"], c2ws, 0.5, 5.0, 10.0)
        for dst in pinned:
            dst[...] = 0  # the call has returned: the engine must not need the caller's images any more
        rb = b.GetResult()
        a.CallAsync(h, w, 7, 5, imgs, big["K"], c2ws, 0.5, 5.0, 10.0)
        ra = a.GetResult()
        for name in ("depth", "confidence", "depth_dense", "confidence_dense"):
            assert np.array_equal(getattr(ra, name).view(np.uint32), getattr(rb, name).view(np.uint32)), (k, name)
    st = b.feature_cache_stats()
    assert st["views_from_cache"] == 6 * (n - 1) and st["key_collisions"] == 0, st
    a.close(); b.close()


@pytest.mark.parametrize("views,capacity,stride", [(7, 8, 1), (7, 9, 2), (4, 5, 1), (3, 12, 3)])
def test_feature_cache_eviction_and_batch_windows(trained_blob, views, capacity, stride):
    """The cache at its edges: the smallest legal capacity (view count + 1: every new image evicts the least recently used entry that the window does not use), windows that
    bring TWO or more new images (computed as a batch, which refills the cache), other view counts, and windows that share nothing with the last one -- always the maps of an
    engine without a cache, bit for bit; the counters say which path every window took."""
    from synth import scene
    from tandem_amd.dr_mvsnet import DrMvsnet
    h, w, n = 96, 160, 6
    big = scene.make_window(h, w, views + stride * (n - 1), seed=37)
    a, b = DrMvsnet(trained_blob), DrMvsnet(trained_blob)
    b.set_feature_cache(capacity)
    for k in range(n):
        lo = k * stride
        imgs = [np.ascontiguousarray(x) for x in big["bgrs"][lo:lo + views]]
        c2ws = list(big["c2ws"][lo:lo + views])
        outs = []
        for m in (a, b):
            m.CallAsync(h, w, views, views - 2, imgs, big["K"], c2ws, 0.5, 5.0, 10.0)
            outs.append(m.GetResult())
        for name in ("depth", "confidence", "depth_dense", "confidence_dense"):
            assert np.array_equal(getattr(outs[0], name).view(np.uint32), getattr(outs[1], name).view(np.uint32)), (k, name)
    st = b.feature_cache_stats()
    new_per_window = min(stride, views)
    assert st["key_collisions"] == 0 and st["single_view_plan"], st
    if new_per_window == 1:
        assert st["batch_windows"] == 1 and st["views_from_cache"] == (views - 1) * (n - 1), st
    else:  # two or more new images: every window is a batch window; what it could have reused it recomputed
        assert st["batch_windows"] == n and st["views_from_cache"] == 0, st
    # going BACK to the first window after the slide: with the smallest capacity its images have been evicted (stride 1: n - 1 = 5 evictions >= views - ... ) or not -- either way the maps are right
    imgs = [np.ascontiguousarray(x) for x in big["bgrs"][:views]]
    outs = []
    for m in (a, b):
        m.CallAsync(h, w, views, views - 2, imgs, big["K"], list(big["c2ws"][:views]), 0.5, 5.0, 10.0)
        outs.append(m.GetResult())
    assert np.array_equal(outs[0].depth_dense.view(np.uint32), outs[1].depth_dense.view(np.uint32))
    a.close(); b.close()
