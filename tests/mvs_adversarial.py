"""Inputs no network produces, for the regression and the edge filter run alone -- TEST INFRASTRUCTURE (a plain module).

Imported by
  tests/test_mvs_adversarial_ref.py   (CPU: the fp32 oracle's error on these inputs = E_DEPTH_ADV / E_CONF_ADV of mvs_stage_ref.py, the cap on pixels
                                       whose E[k] lies next to an integer, the two filter references against each other, and every mutant)
  tests/test_mvs_adversarial_gpu.py   (GPU: the kernels behind debug_regress / debug_prob_regress / debug_edge_filter on the same inputs).

REGRESSION.  The pixels of one image are split into eight families (FAMILIES), pixel n belonging to family (n + offset) % 8; logits are float32 values and the
references take exactly those.  The planes are the kernels' PlaneArgs: uniform (prev = None), adaptive around a smooth previous depth, and adaptive with a
third of the previous depth below half_range, where lo is clamped to 1e-3.  delta is a dyadic number, so half_range = D/2 delta and full_range = D delta are
exact in float32 and the float64 planes see the same numbers as the kernel.

EDGE FILTER.  edge_filter_np is a numpy statement of the filter, independent of oracle.mvsnet_oracle: zero-padded windows, np.sort(...)[14],
np.sort(edge.ravel())[rank], edge > threshold.  Non-finite depth is out of scope: a NaN has no rank.  select_keys builds non-negative float keys from bit
patterns for the three-level radix select (key bits [21, 32), [10, 21), [0, 10))."""
import numpy as np

import mvs_stage_ref as R

FAMILIES = ("flat", "one-hot random plane", "one-hot plane 0 / D-1", "wide random", "nearly flat", "large offset", "two adjacent planes", "peak with noise")
ONE_HOT = (1, 2)         # families whose softmax is exactly one-hot in float32: exp(-400) underflows to 0
NEAR_CAP = 0.05          # the share of the other families' pixels that may lie within R.EK_INTEGER_BAND of an integer E[k] (with two different candidates)
REGRESS_D = (48, 32, 8, 4, 16, 5)   # k_regress_r<48/32/8/4>; 16 and 5 run the generic k_regress
REGRESS_HW = (24, 40)               # 960 pixels: three full workgroups of 256 and a partial one
PLANE_KINDS = ("uniform", "adaptive", "clamped")
DMIN, INTERVAL = 0.5, float(np.float32(4.5 / 47))
DELTA = 0.046875         # 3/64: D/2 delta and D delta are exact in float32 for every D used here


# ------------------------------------------------------------------ regression
def adversarial_logits(D, h, w, seed, offset=0):
    """(logits (D, h, w) float32, family (h, w) int)."""
    rng = np.random.default_rng(seed)
    n = h * w
    fam = (np.arange(n) + offset) % 8
    k = np.arange(D, dtype=np.float64)[:, None]
    lg = np.zeros((D, n))
    hot = rng.integers(0, D, n)
    ends = np.where((np.arange(n) // 8) % 2 == 0, 0, D - 1)
    for f, plane in ((1, hot), (2, ends)):
        sel = fam == f
        lg[:, sel] = np.where(k == plane[None, sel], 0.0, -400.0)
    lg[:, fam == 3] = 6.0 * rng.standard_normal((D, n))[:, fam == 3]
    lg[:, fam == 4] = 1e-3 * rng.standard_normal((D, n))[:, fam == 4]
    lg[:, fam == 5] = 1e4 + 3.0 * rng.standard_normal((D, n))[:, fam == 5]
    first = rng.integers(0, max(D - 1, 1), n)
    second = rng.uniform(-3.0, 3.0, n)
    g = np.where(k == first[None], 0.0, np.where(k == first[None] + 1, second[None], -50.0))
    lg[:, fam == 6] = g[:, fam == 6]
    centre = rng.uniform(0.0, D - 1.0, n)
    peak = 6.0 * np.exp(-0.5 * ((k - centre[None]) / 1.2) ** 2) + 0.7 * rng.standard_normal((D, n))
    lg[:, fam == 7] = peak[:, fam == 7]
    return lg.astype(np.float32).reshape(D, h, w), fam.reshape(h, w)


def plane_setup(kind, D, h, w, seed=5):
    """The arguments of debug_regress and the float64 planes of one plane kind: (kwargs, planes64 (D, h, w), planes32 or None).
    planes32: the uniform planes as the kernel computes them, fmaf(interval, k, dmin) in float32, for the bit-for-bit check of the one-hot families."""
    if kind == "uniform":
        p64 = R.uniform_planes64(DMIN, INTERVAL, D, h, w)
        # interval * k is exact in double (24 + 6 bits), the sum with dmin too: one rounding to float = fmaf
        p32 = (float(np.float32(INTERVAL)) * np.arange(D, dtype=np.float64) + float(np.float32(DMIN))).astype(np.float32)
        return dict(dmin=DMIN, interval=INTERVAL), p64, p32
    hp, wp = h // 2, w // 2
    half, full = (D / 2.0) * DELTA, D * DELTA
    assert float(np.float32(half)) == half and float(np.float32(full)) == full
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(hp) / max(hp, 1), np.arange(wp) / max(wp, 1), indexing="ij")
    prev = 2.0 + 0.6 * np.sin(3.0 * xs + 1.0) * np.cos(2.0 * ys) + 0.3 * ys   # smooth, well above every half_range (<= 1.125)
    if kind == "clamped":   # a third of the previous depth below half_range: lo = max(cur - half_range, 1e-3) clamps there
        low = np.broadcast_to(np.arange(hp)[:, None] < (hp + 2) // 3, (hp, wp))   # (the top rows: the upsampling mixes neighbours)
        prev = np.where(low, half * rng.uniform(0.1, 0.9, (hp, wp)), prev)
    else:
        assert kind == "adaptive", kind
    prev = prev.astype(np.float32)
    return dict(prev=prev, half_range=half, full_range=full), R.adaptive_planes64(prev, D, DELTA, h, w), None


def regression_cases():
    """(id, D, h, w, plane kind, family offset): every D at 24 x 40 with the three plane kinds, and at 2 x 2 with a 1 x 1 prev (every tap of the x2
    upsampling clamped; two offsets so that the four pixels see all eight families)."""
    cases = []
    for D in REGRESS_D:
        for kind in PLANE_KINDS:
            cases.append(("D%d-%dx%d-%s" % (D, REGRESS_HW[0], REGRESS_HW[1], kind), D, REGRESS_HW[0], REGRESS_HW[1], kind, 0))
        for kind, off in (("adaptive", 0), ("clamped", 4)):
            cases.append(("D%d-2x2-%s-o%d" % (D, kind, off), D, 2, 2, kind, off))
    return cases


def regression_inputs(case):
    """(logits, family, debug_regress kwargs, planes64, planes32 or None) of one regression_cases() entry."""
    _, D, h, w, kind, off = case
    logits, fam = adversarial_logits(D, h, w, seed=1000 + D + 7 * h, offset=off)
    kw, p64, p32 = plane_setup(kind, D, h, w)
    return logits, fam, kw, p64, p32


def check_regression(depth, conf, logits, fam, planes, planes32=None):
    """What tests/test_mvs_adversarial_gpu.py holds a kernel's (depth, conf) to, as numbers:
      depth_rel, conf_err   maxima over ALL pixels: |depth - d64| / |d64|; |conf - sum4[trunc(E[k])]| -- with conf_error's two-candidate rule where E[k]
                            lies within EK_INTEGER_BAND of an integer, except in the one-hot families, which use plain index equality
      conf_not_one          one-hot pixels whose conf is not exactly 1.0
      depth_bits            one-hot pixels whose depth is not the float32 plane value bit for bit (uniform planes: planes32 given), else 0
      near_share            of the pixels outside the one-hot families, the share where the two-candidate rule applies AND the candidates differ
    (NaN in depth_rel / conf_err if the outputs hold one)."""
    depth, conf = np.asarray(depth), np.asarray(conf)
    d64, ek, sum4 = R.regress64(logits, planes)
    rel = np.abs(depth.astype(np.float64) - d64) / np.abs(d64)
    cerr, near = R.conf_error(conf.astype(np.float64), ek, sum4)
    onehot = np.isin(fam, ONE_HOT)
    strict = np.abs(conf.astype(np.float64) - R.conf_at(sum4, np.trunc(ek)))
    cerr = np.where(onehot, strict, cerr)
    r = np.rint(ek)
    differ = R.conf_at(sum4, r - 1) != R.conf_at(sum4, r)
    res = dict(depth_rel=float(np.max(rel)), conf_err=float(np.max(cerr)), conf_not_one=int((onehot & (conf != 1.0)).sum()), depth_bits=0,
               near_share=float((near & differ & ~onehot).sum()) / max(int((~onehot).sum()), 1))
    if planes32 is not None:
        want = np.asarray(planes32, np.float32)[np.argmax(logits, axis=0)]
        res["depth_bits"] = int((onehot & (depth.astype(np.float32).view(np.uint32) != want.view(np.uint32))).sum())
    return res


def regression_verdict(res, e_depth, e_conf):
    """The list of violated checks of one check_regression result against BOUND_FACTOR x the recorded reference errors (empty: the kernel passes)."""
    bad = []
    if not res["depth_rel"] <= R.BOUND_FACTOR * e_depth:
        bad.append("depth rel %.3e > %.3e" % (res["depth_rel"], R.BOUND_FACTOR * e_depth))
    if not res["conf_err"] <= R.BOUND_FACTOR * e_conf:
        bad.append("conf %.3e > %.3e" % (res["conf_err"], R.BOUND_FACTOR * e_conf))
    if res["conf_not_one"]:
        bad.append("%d one-hot pixels with conf != 1.0" % res["conf_not_one"])
    if res["depth_bits"]:
        bad.append("%d one-hot pixels whose depth is not the plane value bit for bit" % res["depth_bits"])
    return bad


# ------------------------------------------------------------------ edge measure + filter
FILTER_SHAPES = ((1, 1), (3, 7), (16, 16), (17, 31), (32, 96))
DEPTH_MAPS = ("constant", "halves", "quantised", "checkerboard", "holes", "tiny", "huge")
DISCARDS = (0.0, 2.5, 50.0, 100.0)
# deliberate one-line mistakes of the FILTER restatement (edge_filter_np / select_np)
FILTER_MUTANTS = ("ge", "rank_minus_1", "rank_plus_1", "order_14th", "order_16th", "replicate_padding", "top22")


def depth_map(kind, H, W, seed=9):
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    ramp = 1.0 + 0.7 * xs + 0.4 * ys + 0.05 * np.sin(9.0 * xs + 4.0 * ys)
    if kind == "constant":
        d = np.full((H, W), 1.5)
    elif kind == "halves":
        d = np.where(xs < 0.5, 1.0, 2.0)
    elif kind == "quantised":   # 8 levels: heavy ties
        d = 1.0 + np.floor(8.0 * (ramp - ramp.min()) / max(ramp.max() - ramp.min(), 1e-9) * 0.999) / 8.0
    elif kind == "checkerboard":
        d = np.where((np.arange(H)[:, None] + np.arange(W)[None]) % 2 == 0, 1.0, 1.5)
    elif kind == "holes":       # a smooth ramp with 10 % zeros
        d = np.where(rng.uniform(size=(H, W)) < 0.1, 0.0, ramp)
    elif kind == "tiny":        # edge values at the low end of the exponent range
        d = ramp * 1e-30
    elif kind == "huge":        # ... and at the high end; every difference stays finite
        d = ramp * 1e30
    else:
        raise ValueError(kind)
    return d.astype(np.float32)


def plan_rank(H, W, discard):
    """The quantile rank as plan_geometry computes it: float32 arithmetic, truncation, clamp to 0 .. n - 1."""
    cut = np.float32(H * W) * (np.float32(100.0) - np.float32(discard))
    cut = np.float32(cut) / np.float32(100.0)
    return int(min(max(int(cut), 0), H * W - 1))


def tie_ranks(sorted_values, at):
    """Ranks of the first and the last element of the run of equal values that contains sorted_values[at], and the ranks one to either side of the run."""
    s = np.asarray(sorted_values)
    n = s.size
    first, last = int(np.searchsorted(s, s[at], "left")), int(np.searchsorted(s, s[at], "right")) - 1
    return sorted({r for r in (first - 1, first, last, last + 1) if 0 <= r < n})


def filter_ranks(edge):
    """Every rank a depth-map case runs: the four discard percentages and the ends of, and the neighbours of, the tie run at the median."""
    H, W = edge.shape
    s = np.sort(edge.ravel())
    return sorted(set(plan_rank(H, W, d) for d in DISCARDS) | set(tie_ranks(s, s.size // 2)))


def edge_measure_np(depth, order=14, padding="zero"):
    d = np.asarray(depth, np.float32)
    H, W = d.shape
    p = np.pad(d, 2, mode="edge" if padding == "replicate" else "constant")
    win = np.stack([p[dy:dy + H, dx:dx + W] for dy in range(5) for dx in range(5)])
    with np.errstate(over="ignore"):
        return np.sort(np.abs(win - d[None]), axis=0)[order]


def select_np(keys, rank, mutant=None):
    """Bits of the rank-th smallest key (non-negative floats, ordered as their bit patterns)."""
    s = np.sort(np.ascontiguousarray(keys, np.float32).ravel().view(np.uint32))
    rank = {"rank_minus_1": max(rank - 1, 0), "rank_plus_1": min(rank + 1, s.size - 1)}.get(mutant, rank)
    bits = int(s[rank])
    return bits & 0xFFFFFC00 if mutant == "top22" else bits


def apply_np(edge, thr_bits, depth, conf, mutant=None):
    thr = np.array([thr_bits], np.uint32).view(np.float32)[0]
    e = np.asarray(edge, np.float32)
    mask = e >= thr if mutant == "ge" else e > thr
    return np.where(mask, np.float32(0), np.asarray(depth, np.float32)), np.where(mask, np.float32(0), np.asarray(conf, np.float32))


def edge_filter_np(depth, conf, rank, mutant=None, edge_in=None):
    """(edge, threshold bits, filtered depth, filtered conf); edge_in replaces the edge measure (the select alone); mutant: one of FILTER_MUTANTS."""
    assert mutant is None or mutant in FILTER_MUTANTS, mutant
    if edge_in is not None:
        edge = np.ascontiguousarray(edge_in, np.float32)
    else:
        edge = edge_measure_np(depth, {"order_14th": 13, "order_16th": 15}.get(mutant, 14), "replicate" if mutant == "replicate_padding" else "zero")
    thr = select_np(edge, rank, mutant)
    d, c = apply_np(edge, thr, depth, conf, mutant)
    return edge, thr, d, c


def same_filter_result(a, b):
    """Bit for bit: edge, threshold bits, depth, conf."""
    return (np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and int(a[1]) == int(b[1]) and
            np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)) and np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32)))


# ------------------------------------------------------------------ the radix select alone
SELECT_N = ((1, 1, 1), (255, 15, 17), (256, 16, 16), (257, 1, 257), (4099, 4099, 1), (40000, 200, 200))  # (n, H, W); 40000 > 128 * 256: k_hist's grid-stride loop
KEY_PATTERNS = ("all_equal", "all_zero_but_one", "top11_shared", "top22_shared", "last_bin", "bin_zero", "denormals", "exponent_spread")


def select_keys(pattern, n, seed=21):
    """n non-negative float32 keys built from bit patterns."""
    rng = np.random.default_rng(seed + n)
    r32 = lambda bits: rng.integers(0, 1 << bits, n, dtype=np.uint64).astype(np.uint32)  # noqa: E731
    top = np.uint32(0x1FC << 21)   # key bits [21, 32) of 1.0 (0x3F800000); 0x1FD << 21 is 1.25
    if pattern == "all_equal":
        k = np.full(n, 0x3F800000, np.uint32)
    elif pattern == "all_zero_but_one":
        k = np.zeros(n, np.uint32)
        k[int(rng.integers(0, n))] = 0x40490FDB
    elif pattern == "top11_shared":
        k = top | r32(21)
    elif pattern == "top22_shared":   # only level 2 discriminates
        k = top | np.uint32(0x2AB << 10) | r32(10)
    elif pattern == "last_bin":       # the median's key: mid field 0x7FF and low field 0x3FF, the last bin of levels 1 and 2
        K = top | np.uint32(0x7FF << 10) | np.uint32(0x3FF)
        u = rng.uniform(size=n)
        k = np.where(u < 0.4, top | r32(21), np.where(u < 0.65, K, np.uint32(0x1FD << 21) | r32(21))).astype(np.uint32)
        k[n // 2] = K
        if n > 2:
            k[0], k[n - 1] = top, np.uint32(0x1FD << 21)   # one key below and one above, so that K sits at the median of small sets as well
    elif pattern == "bin_zero":       # the median's key is +0.0: bin 0 of every level
        k = np.where(rng.uniform(size=n) < 0.6, np.uint32(0), np.uint32(1) + r32(30)).astype(np.uint32)
        k[n // 2] = 0
    elif pattern == "denormals":
        k = np.uint32(1) + (r32(23) % np.uint32(0x7FFFFF))
    elif pattern == "exponent_spread":
        k = (rng.integers(1, 255, n, dtype=np.uint64).astype(np.uint32) << np.uint32(23)) | r32(23)
    else:
        raise ValueError(pattern)
    k = np.ascontiguousarray(k, np.uint32)
    assert (k < 0x7F800000).all()
    return k.view(np.float32)


def select_ranks(keys):
    """0, n - 1, n / 2 and both ends of the longest run of equal keys."""
    s = np.sort(np.ascontiguousarray(keys, np.float32).ravel().view(np.uint32))
    n = s.size
    vals, start, counts = np.unique(s, return_index=True, return_counts=True)
    i = int(np.argmax(counts))
    return sorted({0, n - 1, n // 2, int(start[i]), int(start[i] + counts[i] - 1)})
