"""-m gpu: the last two operators of the depth pipeline -- the soft-argmax regression and the edge filter -- run ALONE (debug_regress, debug_prob_regress,
debug_edge_filter: the engine's own launchers and kernel choice on buffers of their own, outputs poisoned) on inputs no network produces
(tests/mvs_adversarial.py), against float64 or exact references.  tests/test_mvs_adversarial_ref.py (CPU) measures the bounds, shows that the two filter
references agree and that every listed one-line mistake fails the checks below on these very inputs.

  regression   k_regress_r<48/32/8/4>, the generic k_regress (D = 16, 5, and DR_REGRESS_GENERIC=1 in the parity build) at 24 x 40 (three workgroups and a partial
               one) and 2 x 2 with a 1 x 1 prev; eight logit families per image, among them a softmax whose largest logit is 1e4, exact one-hot rows on plane 0
               and D-1 (the confidence window clipped on either side) and planes clamped at 1e-3.  Depth relative and confidence absolute within
               BOUND_FACTOR x E_DEPTH_ADV / E_CONF_ADV of regress64, no pixel excluded; the one-hot families bit for bit: conf == 1.0, depth == the float32 plane.
  prob head    k_prob2_regress<8> with a prob weight that copies channel 0: its logits are the input's, its depth / conf the bits of debug_regress on them.
  edge filter  from depth maps with ties, zeros and edge values at both ends of the exponent range, at every rank where > and >= or rank +- 1 differ:
               edge, threshold bits, depth, conf bit for bit against oracle.mvsnet_oracle AND against the numpy statement edge_filter_np.
  radix select alone (edge_in): keys built from bit patterns -- equal in their top 11 or 22 bits, the rank's key in the last or the first bin of every level,
               denormals -- for n = 1 .. 40000 (beyond 128 x 256: the grid-stride loop), DR_FILTER_FUSED 1 / 0, DR_HIST_BLOCKS 128 / 1.
  footprint    one case of each under guarded allocations: nothing written outside a buffer, the same bits as unguarded.

Non-finite depth is out of scope: a NaN has no rank.  Measured on an MI355X (DESIGN.md section 4 has the table)."""
import numpy as np
import pytest

import guard_helpers as G
import mvs_adversarial as A
import mvs_stage_ref as R

pytestmark = pytest.mark.gpu

SWITCHES = ("DR_REGRESS_GENERIC", "DR_PROB_ZCHUNK", "DR_PROB_REGRESS", "DR_FILTER_FUSED", "DR_HIST_BLOCKS", "DR_PROB_V1", "DR_PROB_ROWS")


@pytest.fixture
def env(monkeypatch):
    """set(NAME=value, ...): exactly these of the switches the hooks read, the others unset."""
    def set_(**kw):
        for n in SWITCHES:
            monkeypatch.delenv(n, raising=False)
        for n, v in kw.items():
            assert n in SWITCHES, n
            monkeypatch.setenv(n, str(v))
    set_()
    return set_


def _library(request, library):
    if library == "parity":
        request.getfixturevalue("parity_hooks")


def _regress_kernel(D, generic=False):
    return "k_regress_r<%d>" % D if D in (48, 32, 8, 4) and not generic else "k_regress"


def _hold_regression(tag, kernel, depth, conf, logits, fam, p64, p32):
    G.assert_no_nan(depth, tag + " depth")
    G.assert_no_nan(conf, tag + " conf")
    res = A.check_regression(depth, conf, logits, fam, p64, p32)
    print("%-34s %-16s depth %.3e (%.2f of its bound)  conf %.3e (%.2f)  near-integer share %.4f" % (
        tag, kernel, res["depth_rel"], res["depth_rel"] / (R.BOUND_FACTOR * R.E_DEPTH_ADV), res["conf_err"], res["conf_err"] / (R.BOUND_FACTOR * R.E_CONF_ADV),
        res["near_share"]))
    bad = A.regression_verdict(res, R.E_DEPTH_ADV, R.E_CONF_ADV)
    assert not bad, "%s (%s): %s" % (tag, kernel, "; ".join(bad))


# ------------------------------------------------------------------ regression
REGRESS = [(c, "product") for c in A.regression_cases()] + [(c, "generic") for c in A.regression_cases() if c[1] in (48, 32, 8, 4) and c[2] > 2]


@pytest.mark.parametrize("case,form", REGRESS, ids=["%s-%s" % (c[0], f) for c, f in REGRESS])
def test_regression_alone_against_float64(case, form, env, request):
    """form product: the product library, the kernel that follows from D.  form generic: the parity build with DR_REGRESS_GENERIC=1 -- k_regress on the plane
    counts that otherwise run k_regress_r<D> -- held to the same bounds and, as mvs_kernels.h claims, bit-identical to the register form."""
    from tandem_amd.dr_mvsnet import debug_regress
    _, D, h, w, kind, off = case
    logits, fam, kw, p64, p32 = A.regression_inputs(case)
    if form == "generic":
        _library(request, "parity")
        env(DR_REGRESS_GENERIC=1)
    depth, conf, kernel = debug_regress(logits, **kw)
    assert kernel == _regress_kernel(D, form == "generic"), kernel
    _hold_regression(case[0] + "-" + form, kernel, depth, conf, logits, fam, p64, p32)
    if form == "generic":
        env()
        d2, c2, k2 = debug_regress(logits, **kw)
        assert k2 == _regress_kernel(D), k2
        G.assert_same_bits(depth, d2, "depth: k_regress against " + k2)
        G.assert_same_bits(conf, c2, "conf: k_regress against " + k2)


# ------------------------------------------------------------------ prob head + regression in one launch
def _prob_inputs(h, w):
    logits, fam = A.adversarial_logits(8, h, w, seed=77 + h)
    x11 = np.random.default_rng(h * w).standard_normal((8, h, w, 8)).astype(np.float32)
    x11[..., 0] = logits
    wp = np.zeros((1, 8, 3, 3, 3), np.float32)
    wp[0, 0, 1, 1, 1] = 1.0   # the centre tap of channel 0: the logits are channel 0, every other product is an exact zero
    return logits, fam, x11, wp


PROB_FORMS = {  # form: (library, switches, kernel names)
    "one-launch-product": ("product", dict(DR_PROB_ZCHUNK=8), "k_prob2_regress<8>"),
    "one-launch-parity": ("parity", dict(DR_PROB_ZCHUNK=8), "k_prob2_regress<8>"),
    "two-launches-default-chunk": ("product", dict(), "k_prob2<1>+k_regress_r<8>"),   # small frames: the default z chunk is 2
    "two-launches-switched-off": ("parity", dict(DR_PROB_ZCHUNK=8, DR_PROB_REGRESS=0), "k_prob2<1>+k_regress_r<8>"),
}


@pytest.mark.parametrize("form", list(PROB_FORMS))
@pytest.mark.parametrize("h,w", [(24, 40), (16, 64)], ids=["24x40", "16x64"])
def test_prob_head_and_regression_in_one_launch(h, w, form, env, request):
    """D = 8: logits_out is channel 0 of the input elementwise; depth / conf are the bits of debug_regress on the same logits (the claim of k_prob2_regress's
    comment) and inside the float64 bound -- on uniform planes (the one-hot families bit for bit) and on planes clamped at 1e-3."""
    from tandem_amd.dr_mvsnet import debug_prob_regress, debug_regress
    library, switches, names = PROB_FORMS[form]
    _library(request, library)
    logits, fam, x11, wp = _prob_inputs(h, w)
    for kind in ("uniform", "clamped"):
        kw, p64, p32 = A.plane_setup(kind, 8, h, w)
        env(**switches)
        lg, depth, conf, kernel = debug_prob_regress(x11, wp, **kw)
        assert kernel == names, kernel
        assert np.array_equal(lg, logits), "%d logits differ from channel 0" % int((lg != logits).sum())
        tag = "prob-%dx%d-%s-%s" % (h, w, kind, form)
        _hold_regression(tag, kernel, depth, conf, logits, fam, p64, p32)
        d2, c2, k2 = debug_regress(logits, **kw)
        assert k2 == "k_regress_r<8>", k2
        G.assert_same_bits(depth, d2, tag + " depth against debug_regress")
        G.assert_same_bits(conf, c2, tag + " conf against debug_regress")


# ------------------------------------------------------------------ edge measure + filter from a depth map
FILTER_FORMS = {"product": ("product", dict()), "parity-scan-launches": ("parity", dict(DR_FILTER_FUSED=0))}


def _conf(H, W):
    return np.random.default_rng(H * 100 + W).uniform(0.1, 1.0, (H, W)).astype(np.float32)


def _same(tag, got, want, ref):
    edge, d, c, thr = got
    G.assert_no_nan(edge, tag + " edge")
    G.assert_no_nan(d, tag + " depth")
    G.assert_no_nan(c, tag + " conf")
    assert np.array_equal(edge.view(np.uint32), want[0].view(np.uint32)), "%s: %d edge values differ from %s" % (tag, int((edge.view(np.uint32) != want[0].view(np.uint32)).sum()), ref)
    assert thr == int(want[1]), "%s: threshold bits %#010x, %s has %#010x" % (tag, thr, ref, int(want[1]))
    assert np.array_equal(d.view(np.uint32), want[2].view(np.uint32)), "%s: %d depth values differ from %s" % (tag, int((d.view(np.uint32) != want[2].view(np.uint32)).sum()), ref)
    assert np.array_equal(c.view(np.uint32), want[3].view(np.uint32)), "%s: %d conf values differ from %s" % (tag, int((c.view(np.uint32) != want[3].view(np.uint32)).sum()), ref)


@pytest.mark.parametrize("form", list(FILTER_FORMS))
@pytest.mark.parametrize("kind", A.DEPTH_MAPS)
@pytest.mark.parametrize("H,W", A.FILTER_SHAPES, ids=["%dx%d" % s for s in A.FILTER_SHAPES])
def test_edge_filter_alone_is_exact(H, W, kind, form, env, request):
    """Every rank of filter_ranks (the four discard percentages through plan_geometry's float32 rule; both ends of the run of ties at the median and the ranks
    next to it): edge, threshold bits, depth and conf bit for bit against the oracle and against edge_filter_np."""
    import torch
    from oracle import mvsnet_oracle as O
    from tandem_amd.dr_mvsnet import debug_edge_filter
    library, switches = FILTER_FORMS[form]
    _library(request, library)
    env(**switches)
    depth, conf = A.depth_map(kind, H, W), _conf(H, W)
    edge_o = O.edge_measure(torch.from_numpy(depth))
    srt, _ = torch.sort(edge_o.reshape(-1))
    ranks = A.filter_ranks(A.edge_measure_np(depth))
    masked = []
    for rank in ranks:
        tag = "%s-%dx%d-%s rank %d" % (kind, H, W, form, rank)
        got = debug_edge_filter(depth, conf, rank)
        mask_o = (edge_o > srt[rank]).numpy()
        want_o = (edge_o.numpy(), int(srt[rank].numpy().view(np.uint32)), np.where(mask_o, np.float32(0), depth), np.where(mask_o, np.float32(0), conf))
        _same(tag, got, want_o, "the oracle")
        _same(tag, got, A.edge_filter_np(depth, conf, rank), "edge_filter_np")
        masked.append(int(mask_o.sum()))
    print("%s-%dx%d-%s: ranks %s, masked %s" % (kind, H, W, form, ranks, masked))


# ------------------------------------------------------------------ the radix select alone
SELECT_FORMS = {"product": ("product", dict()), "parity-fused": ("parity", dict(DR_FILTER_FUSED=1)), "parity-scan-launches": ("parity", dict(DR_FILTER_FUSED=0))}


@pytest.mark.parametrize("blocks", [128, 1])
@pytest.mark.parametrize("form", list(SELECT_FORMS))
@pytest.mark.parametrize("n,H,W", A.SELECT_N, ids=["n%d" % s[0] for s in A.SELECT_N])
def test_radix_select_alone_is_exact(n, H, W, form, blocks, env, request):
    """edge_in: the select and the mask on chosen keys.  Threshold bits == np.sort(keys as uint32)[rank]; depth / conf zeroed exactly where key > threshold."""
    from tandem_amd.dr_mvsnet import debug_edge_filter
    library, switches = SELECT_FORMS[form]
    _library(request, library)
    env(DR_HIST_BLOCKS=blocks, **switches)
    depth = np.random.default_rng(n).uniform(0.5, 2.0, (H, W)).astype(np.float32)
    conf = _conf(H, W)
    for pattern in A.KEY_PATTERNS:
        keys = A.select_keys(pattern, n).reshape(H, W)
        s = np.sort(keys.ravel().view(np.uint32))
        for rank in A.select_ranks(keys):
            tag = "%s n %d %s blocks %d rank %d" % (pattern, n, form, blocks, rank)
            got = debug_edge_filter(depth, conf, rank, edge_in=keys)
            assert got[3] == int(s[rank]), "%s: threshold bits %#010x, sorted keys have %#010x" % (tag, got[3], int(s[rank]))
            _same(tag, got, A.edge_filter_np(depth, conf, rank, edge_in=keys), "edge_filter_np")


# ------------------------------------------------------------------ footprint: the same calls between guard bands
def test_footprint_regression(env, parity_hooks):
    from tandem_amd.dr_mvsnet import debug_regress
    case = [c for c in A.regression_cases() if c[0] == "D48-24x40-clamped"][0]
    logits, fam, kw, p64, p32 = A.regression_inputs(case)
    plain = debug_regress(logits, **kw)
    with G.guarded():
        held = debug_regress(logits, **kw)
    G.assert_same_bits(held[0], plain[0], "regression depth")
    G.assert_same_bits(held[1], plain[1], "regression conf")


def test_footprint_prob_regress(env, parity_hooks):
    from tandem_amd.dr_mvsnet import debug_prob_regress
    logits, fam, x11, wp = _prob_inputs(24, 40)
    kw, p64, p32 = A.plane_setup("clamped", 8, 24, 40)
    env(DR_PROB_ZCHUNK=8)
    plain = debug_prob_regress(x11, wp, **kw)
    with G.guarded():
        held = debug_prob_regress(x11, wp, **kw)
    assert plain[3] == held[3] == "k_prob2_regress<8>"
    for i, what in enumerate(("logits", "depth", "conf")):
        G.assert_same_bits(held[i], plain[i], "prob + regression " + what)


@pytest.mark.parametrize("which", ["depth-17x31", "keys-n4099"])
def test_footprint_edge_filter(which, env, parity_hooks):
    from tandem_amd.dr_mvsnet import debug_edge_filter
    if which == "depth-17x31":
        depth, conf, keys = A.depth_map("holes", 17, 31), _conf(17, 31), None
        rank = A.plan_rank(17, 31, 2.5)
    else:
        depth, conf = A.depth_map("quantised", 4099, 1), _conf(4099, 1)
        keys = A.select_keys("top22_shared", 4099).reshape(4099, 1)
        rank = 4099 // 2
    plain = debug_edge_filter(depth, conf, rank, edge_in=keys)
    with G.guarded():
        held = debug_edge_filter(depth, conf, rank, edge_in=keys)
    for i, what in enumerate(("edge", "depth", "conf")):
        G.assert_same_bits(held[i], plain[i], "edge filter " + what)
    assert held[3] == plain[3]
