"""-m gpu: the parts of the DrMvsnet engine (tandem_amd/csrc/mvs_stage.h WindowStager, mvs_cache.h FeatureCacheDev, mvs_shard.h ViewShard's phase
mode, mvs_engine_host.h ResultSlots / WindowTicket / ForwardCursor) on ONE engine with the feature cache on, through every path that shares state
between them, in one sequence.  Each path has a test of its own elsewhere (tests/test_mvsnet_gpu.py, tests/test_view_shard_gpu.py); what is
checked here is that none of them leaves something behind that the next one trips over.  64x96 windows of 4 views, cache capacity 5.

After every step the four maps equal those of a fresh engine without a cache bit for bit, and drm_feature_cache_stats equals what the windows
so far imply (the counting rule: mvs_host.h FeatureIndex::plan -- a window with at most one unknown image counts its known images as served
from the cache and the unknown one as computed; any other window is a batch window that computes all its views; staging a window counts,
running it again does not; a hit that the device compare refutes is one collision and drops every entry)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAPS = ("depth", "confidence", "depth_dense", "confidence_dense")
H, W, V, CAP = 64, 96, 4, 5
RANGE = (0.5, 5.0, 10.0)


def _same(x, y, what):
    for name in MAPS:
        a, b = getattr(x, name), getattr(y, name)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, name, np.abs(a - b).max())


def test_one_engine_through_every_path_that_shares_state(trained_blob):
    from synth import scene
    from tandem_amd import _lib
    from tandem_amd.dr_mvsnet import DrMvsnet

    big = scene.make_window(H, W, V + 3, seed=43)
    imgs = [np.ascontiguousarray(x) for x in big["bgrs"]]
    c2ws = list(big["c2ws"])
    ref_index = V - 2

    def args(lo, images=None, h=H, w=W, K=None, poses=None):
        return (h, w, V, ref_index, images if images is not None else imgs[lo:lo + V], big["K"] if K is None else K,
                c2ws[lo:lo + V] if poses is None else poses) + RANGE

    def fresh(a):
        """the window on a fresh engine without a cache, through the reference's calls"""
        m = DrMvsnet(trained_blob)
        m.CallAsync(*a)
        out = m.GetResult()
        m.close(force=True)
        return out

    b = DrMvsnet(trained_blob)
    b.set_feature_cache(CAP)
    want = dict(views_from_cache=0, views_computed=0, batch_windows=0, key_collisions=0, single_view_plan=False, entries=0)
    assert b.feature_cache_stats() == want  # (not configured yet: no plan, no entries)

    # 1. a batch window: nothing is cached, all four views are computed and fill the cache
    b.CallAsync(*args(0))
    _same(b.GetResult(), fresh(args(0)), "batch window")
    want.update(views_computed=4, batch_windows=1, single_view_plan=True, entries=CAP)
    assert b.feature_cache_stats() == want
    with pytest.raises(_lib.DrError) as e:  # GetResult twice: the existing protocol error
        b.GetResult()
    assert e.value.code == 2 and "Output should be valid. Maybe you called GetResult more than once?" in str(e.value)

    # 2. two sliding windows through CallAsync (three known images, one new: the calling thread enqueues the forward itself) ...
    b.CallAsync(*args(1))
    _same(b.GetResult(), fresh(args(1)), "sliding window")
    want.update(views_from_cache=3, views_computed=5)
    assert b.feature_cache_stats() == want
    # ... the second with page-locked images, uploaded in place and overwritten as soon as the call has returned
    pinned = b.alloc_images(V, H, W)
    for dst, src in zip(pinned, imgs[2:2 + V]):
        dst[...] = src
    b.CallAsync(*args(2, images=pinned))
    for dst in pinned:
        dst[...] = 0
    _same(b.GetResult(), fresh(args(2)), "sliding window, page-locked")
    want.update(views_from_cache=6, views_computed=6)
    assert b.feature_cache_stats() == want

    # the same window through the hooks on a fresh engine without a cache: the reference of steps 3 to 5
    r = DrMvsnet(trained_blob)
    r.upload(*args(2)); r.forward(1)
    hook_ref, feat1_ref, rows_ref = r.download(), r.tensor("feat1").copy(), [(x["op"], x["kernel"]) for x in r.profile()]
    r.close(force=True)

    # 3. upload + forward(2) on the same window: every image is known, FeatureNet does not run at all
    b.upload(*args(2)); b.forward(2)
    _same(b.download(), hook_ref, "upload + forward(2)")
    want.update(views_from_cache=10)
    assert b.feature_cache_stats() == want
    assert not np.array_equal(b.tensor("feat1"), feat1_ref)  # (the batch feature maps are still an earlier window's: the sweep read the entries)

    # a second engine created, used and destroyed in the middle changes nothing
    x = DrMvsnet(trained_blob)
    x.CallAsync(*args(0)); x.GetResult()
    x.close(force=True)

    # 4. the four phases of it: a partial forward cannot skip FeatureNet, so the window goes back to the batch path
    for p in range(4):
        b.forward_phase(p)
    _same(b.download(), hook_ref, "forward_phase 0..3")
    assert np.array_equal(b.tensor("feat1").view(np.uint32), feat1_ref.view(np.uint32))  # FeatureNet ran over the batch
    assert b.feature_cache_stats() == want  # (no window was staged)
    with pytest.raises(_lib.DrError):  # the hooks publish nothing
        b.GetResult()

    # 5. profile(): the plan's ops and kernels, and the maps once more
    assert [(x["op"], x["kernel"]) for x in b.profile()] == rows_ref
    _same(b.download(), hook_ref, "profile")
    assert b.feature_cache_stats() == want

    # 6. a window whose one image is forged between two sampled words: every key hits, the device compare refutes one
    n = H * W * 3
    step = (n // 512) & ~7
    assert step >= 32
    forged = [x.copy() for x in imgs[2:2 + V]]
    forged[1].reshape(-1)[200 * step + 16: 200 * step + 24] ^= 0x5A  # (words 200 * step and 201 * step are sampled, 8 bytes each)
    b.CallAsync(*args(2, images=forged))
    _same(b.GetResult(), fresh(args(2, images=forged)), "forged image")
    want.update(views_from_cache=14, key_collisions=1)
    assert b.feature_cache_stats() == want

    # 7. the cache off (the engine is re-planned), then a window
    b.set_feature_cache(0)
    want.update(single_view_plan=False, entries=0)
    assert b.feature_cache_stats() == want
    with pytest.raises(_lib.DrError):  # (the result blocks were the old plan's)
        b.GetResult()
    b.CallAsync(*args(3))
    _same(b.GetResult(), fresh(args(3)), "cache off")
    assert b.feature_cache_stats() == want

    # 8. another window shape, then a window
    h2, w2 = 96, 128
    big2 = scene.make_window(h2, w2, V, seed=44)
    a2 = args(0, images=[np.ascontiguousarray(x) for x in big2["bgrs"]], h=h2, w=w2, K=big2["K"], poses=list(big2["c2ws"]))
    b.CallAsync(*a2)
    out = b.GetResult()
    assert out.depth.shape == (h2, w2)
    _same(out, fresh(a2), "shape change")
    assert b.feature_cache_stats() == want
    b.close(force=True)
