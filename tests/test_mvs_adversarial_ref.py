"""CPU: the inputs of tests/test_mvs_adversarial_gpu.py (tests/mvs_adversarial.py) against the references alone.

 * the fp32 oracle's regression against regress64 on the adversarial logits: E_DEPTH_ADV / E_CONF_ADV of mvs_stage_ref.py are MEASURED here (the GPU
   test's bounds are BOUND_FACTOR x them) and must not drift by more than 1.5 x;
 * at most NEAR_CAP of the pixels outside the one-hot families have an E[k] next to an integer where conf_error's two candidates differ: the
   two-candidate rule stays an exception;
 * the two references of the edge filter -- oracle.mvsnet_oracle and the numpy statement edge_filter_np -- agree bit for bit on every depth map and rank;
 * every mutant of the regression, of the planes and of the filter restatement leaves the GPU test's bound or breaks its exact comparison on these very
   inputs: the inputs are not too tame for the test to fail.
"""
import numpy as np
import pytest
import torch

import mvs_adversarial as A
import mvs_stage_ref as R

_CACHE = {}


def _inputs(case):
    if case[0] not in _CACHE:
        _CACHE[case[0]] = A.regression_inputs(case)
    return _CACHE[case[0]]


def test_reference_error_on_the_adversarial_logits_is_measured_and_has_not_drifted():
    """The fp32 oracle (softmax, expectation, avg_pool window, gather) against regress64 on the same logits and planes; prints E_DEPTH_ADV / E_CONF_ADV."""
    from oracle import mvsnet_oracle as O
    e_depth = e_conf = 0.0
    for case in A.regression_cases():
        logits, fam, kw, p64, _ = _inputs(case)
        with torch.no_grad():
            depth, conf = O.regress(torch.from_numpy(logits), torch.from_numpy(p64.astype(np.float32)))
        res = A.check_regression(depth.numpy(), conf.numpy(), logits, fam, p64)
        print("%-22s depth rel %.3e  conf %.3e  near-integer share %.4f" % (case[0], res["depth_rel"], res["conf_err"], res["near_share"]))
        e_depth, e_conf = max(e_depth, res["depth_rel"]), max(e_conf, res["conf_err"])
    print("\nE_DEPTH_ADV = %.2e\nE_CONF_ADV = %.2e" % (e_depth, e_conf))
    assert e_depth <= 1.5 * R.E_DEPTH_ADV and e_conf <= 1.5 * R.E_CONF_ADV, (e_depth, e_conf)


def test_the_two_candidate_rule_stays_an_exception():
    """Outside the one-hot families at most NEAR_CAP of a case's pixels have E[k] within EK_INTEGER_BAND of an integer with two DIFFERENT candidates.
    (With D = 5 the flat family's E[k] is exactly 2 and both candidates are the same p0 + .. + p3 = p1 + .. + p4: the rule gives such a pixel no
    latitude, so it does not count.)  The inputs reach what they are built for: the clamp of lo, both ends of the window, exact one-hot softmaxes."""
    for case in A.regression_cases():
        logits, fam, kw, p64, _ = _inputs(case)
        d64, conf64 = R.regress_out64(logits, p64)
        res = A.check_regression(d64, conf64, logits, fam, p64)
        assert res["near_share"] <= A.NEAR_CAP, (case[0], res["near_share"])
        _, D, h, w, kind, off = case
        if kind == "clamped":
            share = float((p64[0] == 1e-3).mean())
            assert (0.1 < share < 0.7) if h > 2 else share == 1.0, (case[0], share)
        if h > 2:
            _, ek, _ = R.regress64(logits, p64)
            idx = np.trunc(ek)
            assert (idx[fam == 2] == 0).any() and (idx[fam == 2] == D - 1).any(), case[0]
            assert float(logits[:, fam == 5].min()) > 9.9e3, case[0]


def test_one_hot_families_are_exact_in_float32():
    """exp(-400) is 0 in float32: the softmax of the one-hot families is exactly one-hot, which the GPU test's bit-for-bit checks rely on."""
    assert np.exp(np.float32(-400.0)) == 0.0
    logits, fam = A.adversarial_logits(8, 24, 40, seed=1)
    hot = logits[:, np.isin(fam, A.ONE_HOT)]
    assert ((hot == 0).sum(axis=0) == 1).all() and ((hot == -400).sum(axis=0) == 7).all()


@pytest.mark.parametrize("mutant", R.REGRESS_MUTANTS + ("no_lo_clamp",))
def test_every_regression_mutant_fails_the_gpu_checks(mutant):
    """The mutant's (depth, conf) through check_regression / regression_verdict -- the GPU test's own checks and bounds: at least one case must fail, and by a
    wide margin (20 x a bound, a NaN, or an exact comparison)."""
    failed, best = [], 0.0
    for case in A.regression_cases():
        logits, fam, kw, p64, p32 = _inputs(case)
        _, D, h, w, kind, off = case
        if mutant == "no_lo_clamp":
            if kind == "uniform":
                continue
            depth, conf = R.regress_out64(logits, R.adaptive_planes64(kw["prev"], D, A.DELTA, h, w, mutant="no_lo_clamp"))
        else:
            depth, conf = R.regress_out64(logits, p64, mutant=mutant)
        res = A.check_regression(depth, conf, logits, fam, p64)
        if A.regression_verdict(res, R.E_DEPTH_ADV, R.E_CONF_ADV):
            failed.append(case[0])
        worst = max(res["depth_rel"] / (R.BOUND_FACTOR * R.E_DEPTH_ADV), res["conf_err"] / (R.BOUND_FACTOR * R.E_CONF_ADV))
        best = max(best, float("inf") if np.isnan(worst) or res["conf_not_one"] else worst)
    print("\n%s: fails %d of %d cases, up to %.3g x a bound" % (mutant, len(failed), len(A.regression_cases()), best))
    assert failed and best > 20.0, (mutant, failed, best)


def test_the_unmutated_restatement_passes_its_own_checks():
    for case in A.regression_cases():
        logits, fam, kw, p64, p32 = _inputs(case)
        depth, conf = R.regress_out64(logits, p64)
        res = A.check_regression(depth, conf, logits, fam, p64)
        assert not A.regression_verdict(res, R.E_DEPTH_ADV, R.E_CONF_ADV), (case[0], res)


# ------------------------------------------------------------------ edge filter
def _filter_cases():
    for H, W in A.FILTER_SHAPES:
        for kind in A.DEPTH_MAPS:
            depth = A.depth_map(kind, H, W)
            conf = np.random.default_rng(H * 100 + W).uniform(0.1, 1.0, (H, W)).astype(np.float32)
            yield "%s-%dx%d" % (kind, H, W), depth, conf


def test_the_two_filter_references_agree_bit_for_bit():
    """oracle.mvsnet_oracle (unfold + kthvalue, sort, >) against edge_filter_np (padded windows + np.sort) on every depth map, shape and rank; the
    discard percentages go through filter_edges itself, whose cut must be plan_rank's."""
    from oracle import mvsnet_oracle as O
    ranks_run = 0
    for name, depth, conf in _filter_cases():
        assert np.isfinite(depth).all()
        H, W = depth.shape
        td = torch.from_numpy(depth)
        edge_o = O.edge_measure(td).numpy()
        edge_n = A.edge_measure_np(depth)
        assert np.isfinite(edge_n).all(), name
        assert np.array_equal(edge_o.view(np.uint32), edge_n.view(np.uint32)), name
        srt, _ = torch.sort(torch.from_numpy(edge_o).reshape(-1))
        for rank in A.filter_ranks(edge_n):
            thr_o = srt[rank]
            mask_o = (torch.from_numpy(edge_o) > thr_o).numpy()
            e, thr, d, c = A.edge_filter_np(depth, conf, rank)
            assert int(thr_o.numpy().view(np.uint32)) == thr, (name, rank)
            assert np.array_equal(d, np.where(mask_o, np.float32(0), depth)) and np.array_equal(c, np.where(mask_o, np.float32(0), conf)), (name, rank)
            ranks_run += 1
        for disc in A.DISCARDS:
            filt, mask, _, thr_o = O.filter_edges(td, disc)
            e, thr, d, c = A.edge_filter_np(depth, conf, A.plan_rank(H, W, disc))
            assert int(thr_o.numpy().view(np.uint32)) == thr and np.array_equal(filt.numpy(), d), (name, disc)
    print("\n%d (map, rank) pairs" % ranks_run)


def test_the_depth_maps_have_the_ties_and_the_range_they_are_built_for():
    for H, W in ((16, 16), (17, 31), (32, 96)):
        for kind in ("constant", "halves", "quantised", "checkerboard"):
            s = np.sort(A.edge_measure_np(A.depth_map(kind, H, W)).ravel())
            first, last = np.searchsorted(s, s[s.size // 2], "left"), np.searchsorted(s, s[s.size // 2], "right") - 1
            assert last - first >= 8, (kind, H, W, first, last)   # a run of ties across the median
        tiny, huge = A.edge_measure_np(A.depth_map("tiny", H, W)), A.edge_measure_np(A.depth_map("huge", H, W))
        assert 0 < tiny.max() < 1e-29 and 1e29 < huge.max() < np.inf
        assert (A.depth_map("holes", H, W) == 0).mean() > 0.04


def test_the_keys_have_the_bit_patterns_they_are_built_for():
    for n, H, W in A.SELECT_N:
        assert H * W == n
        for pattern in A.KEY_PATTERNS:
            k = A.select_keys(pattern, n).view(np.uint32)
            assert k.size == n and (k < 0x7F800000).all(), (pattern, n)
            s = np.sort(k)
            if pattern == "top11_shared":
                assert len(set(s >> 21)) == 1
            if pattern == "top22_shared":
                assert len(set(s >> 10)) == 1 and (n < 64 or len(set(s)) > 16)
            if pattern == "last_bin":
                assert (int(s[n // 2]) >> 10) & 0x7FF == 0x7FF and int(s[n // 2]) & 0x3FF == 0x3FF, (n, hex(int(s[n // 2])))
            if pattern == "bin_zero":
                assert s[n // 2] == 0
            if pattern == "denormals":
                assert (s > 0).all() and (s < 0x00800000).all()
            if pattern == "exponent_spread" and n >= 4099:
                assert len(set(s >> 23)) > 200
        assert any(n > 128 * 256 for n, _, _ in A.SELECT_N)


@pytest.mark.parametrize("mutant", A.FILTER_MUTANTS)
def test_every_filter_mutant_breaks_the_exact_comparison(mutant):
    """Each mutant of the filter restatement differs from the restatement in edge, threshold bits, depth or conf on at least one of the GPU test's inputs:
    a depth map and rank, or (the select alone) a key pattern and rank."""
    broken = []
    for name, depth, conf in _filter_cases():
        for rank in A.filter_ranks(A.edge_measure_np(depth)):
            if not A.same_filter_result(A.edge_filter_np(depth, conf, rank), A.edge_filter_np(depth, conf, rank, mutant=mutant)):
                broken.append((name, rank))
    for n, H, W in A.SELECT_N:
        depth = np.random.default_rng(n).uniform(0.5, 2.0, (H, W)).astype(np.float32)
        for pattern in A.KEY_PATTERNS:
            keys = A.select_keys(pattern, n).reshape(H, W)
            for rank in A.select_ranks(keys):
                if not A.same_filter_result(A.edge_filter_np(depth, depth, rank, edge_in=keys), A.edge_filter_np(depth, depth, rank, mutant=mutant, edge_in=keys)):
                    broken.append((pattern, n, rank))
    print("\n%s: breaks %d comparisons, e.g. %s" % (mutant, len(broken), broken[:3]))
    assert broken, mutant
    if mutant == "top22":   # only keys that agree in their top 22 bits tell this one apart: the third select level
        assert any(b[0] == "top22_shared" for b in broken), broken[:10]
