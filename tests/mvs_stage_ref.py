"""Float64 restatements of the DrMvsnet stages between FeatureNet and the edge filter -- TEST INFRASTRUCTURE.

One function per stage operation (hypothesis planes, cost volume, prob head, regression, FeatureNet), each a plain
numpy / torch float64 statement of the reference's arithmetic, written independently of oracle/mvsnet_oracle.py: the cost
volume gathers its four taps from a zero-padded map (no grid_sample), the homography comes from double inverses.  They
are imported by
  tests/test_mvs_stage_ref.py    (CPU: the fp32 oracle against these = the reference's own rounding error, and what a
                                  one-line mistake moves)
  tests/test_mvs_stages_gpu.py   (GPU: every stage tensor of the engine against these, fed the engine's own stage input)
  tests/mvs_adversarial.py       (the regression run alone on inputs no network produces: adaptive_planes64 / uniform_planes64, regress64 and its
                                  mutants regress_out64(mutant=); E_DEPTH_ADV / E_CONF_ADV are measured by tests/test_mvs_adversarial_ref.py).

Layouts are the engine's logical ones (DrMvsnet.tensor): feature maps (V, h, w, C), volumes (D, h, w, C), x11 (D, h, w, 8),
logits (D, h, w), planes (D, h, w); views in model order [ref, the others in window order].

THE RECORDED REFERENCE ERRORS (E_*).  The fp32 oracle against the float64 restatement given the oracle's own stage
inputs, maximum over CPU_WINDOWS, as a fraction of the float64 tensor's range max - min (depth: relative; confidence:
absolute, its range is 1).  Produced by
    python -m pytest tests/test_mvs_stage_ref.py -q -s -k reference_error
which prints the block below; tests/test_mvs_stage_ref.py asserts the oracle stays within 1.5 x of it.  The GPU test
holds every kernel to BOUND_FACTOR x these figures: the kernel's coordinate passes a 1-ulp reciprocal and an fp32 matrix
rounded from double, each worth about one more rounding of the size of the reference's own normalise / denormalise round
trip -- a margin over the reference's error, not a number fitted to the kernels.

THE LAYER RESTATEMENTS (the last section).  One function per layer kind of CostRegNet (conv_bn_relu64,
deconv_bn_relu_skip64) and one per FeatureNet tensor the engine keeps (feature_net_layers), each returning the float64 output AND
the float64 value before the ReLU.  A layer's error is taken as a fraction of layer_scale() = max(max |value before the
ReLU|, max |output|): a (6, 1, 1) level behind a ReLU can have a range near zero while its accumulations are O(1), so the
output's range is not used.  The bound is CONV_BOUND of that scale; E_LAYER is the fp32 oracle's own layer against the
restatement given the oracle's own input, in the same unit (tests/test_mvs_stage_ref.py asserts
BOUND_FACTOR * E_LAYER <= CONV_BOUND).  The transposed layers are stated as zero insertion + a plain convolution with the
flipped kernel (no conv_transpose), BatchNorm as its eval formula.  Imported by tests/test_mvs_layers_gpu.py as well.
"""
import numpy as np
import torch
import torch.nn.functional as F

BOUND_FACTOR = 4.0
CONV_BOUND = 2e-5        # the project's convolution bound (tests/test_conv_gpu.py): of the output's range (the logits), of layer_scale() (one layer)
EK_INTEGER_BAND = 1e-4   # trunc(E[k]) is discontinuous: within this distance of an integer either neighbouring index is accepted
                         # (the fp32 sum of <= 48 terms p * k errs by about 48 * 2^-23 * a few = 2e-5)

# --- recorded by the command above (see the module docstring) ---
E_VOL = {1: 4.53e-06, 2: 9.62e-06, 3: 2.87e-05}
E_VOL_MEAN = {1: 8.31e-08, 2: 1.80e-07, 3: 2.47e-07}
E_VOL_PLAIN = {1: 5.20e-06, 2: 1.31e-05, 3: 2.45e-05}       # the plain-variance model (no view aggregation): another operation, its own reference error
E_VOL_PLAIN_MEAN = {1: 8.68e-08, 2: 1.95e-07, 3: 3.69e-07}  # (maximum over test_mvs_stage_ref.PLAIN_WINDOWS)
E_DEPTH = 4.77e-07
E_CONF = 5.64e-07
E_DEPTH_ADV = 6.66e-07  # the same two figures on the adversarial logits of tests/mvs_adversarial.py (regression run alone): recorded by
E_CONF_ADV = 5.70e-07   #     python -m pytest tests/test_mvs_adversarial_ref.py -q -s -k reference_error
E_FEAT = {1: 9.23e-07, 2: 9.44e-07, 3: 9.16e-07}
E_LAYER = 1.72e-06  # one layer (THE LAYER RESTATEMENTS), of layer_scale(): the maximum over CPU_WINDOWS and SMALL_WINDOWS, every CostRegNet and FeatureNet layer
# ---

MUTANTS = ("border", "no_behind_mask", "shift", "no_gate", "drop_last_view", "divisor_V", "spacing_Dm1")
BN_EPS = 1e-5


# ------------------------------------------------------------------ windows
def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    R = np.eye(4)
    i, j = {"x": (1, 2), "y": (2, 0), "z": (0, 1)}[axis]
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


POSES = ("scene", "narrow", "behind", "rotated")


def make_case(height, width, views, pose, seed=3):
    """A synth.scene window in one of the four pose / range settings:
      scene    the scene's own poses, depth range 0.5 .. 5
      narrow   the same poses, 0.3 .. 1.2 (sub-pixel steps between planes)
      behind   0.01 .. 10 with the first source camera moved 0.05 m AHEAD of the reference along its z axis: the first
               hypothesis plane (and every adaptive plane clamped at 1e-3) lies behind that camera, pz < 0.001; with three
               views or more the second source stands 1.4 m ahead, which puts stage-3 planes behind a camera too
      rotated  the reference camera rolled by 0.5 rad about its optical axis and yawed by 0.12 rad: about a quarter of the
               samples leave the source images, through all four borders
    (the images stay those of the scene: parity does not need consistent geometry).  Returns the window dict with
    depth_min / depth_max set."""
    from synth import scene
    win = dict(scene.make_window(height, width, views, seed=seed))
    c2ws = np.array(win["c2ws"], np.float64)
    ref = win["ref_index"]
    dmin, dmax = 0.5, 5.0
    if pose == "narrow":
        dmin, dmax = 0.3, 1.2
    elif pose == "behind":
        dmin, dmax = 0.01, 10.0
        srcs = [i for i in range(views) if i != ref]
        c2ws[srcs[0], :3, 3] = c2ws[ref, :3, 3] + c2ws[ref, :3, :3] @ np.array([0.01, -0.005, 0.05])
        if len(srcs) > 1:  # stage 3's planes lie within 0.2 m of the stage-2 depth (1.3 .. 2.4 m in this scene): a camera between the slab and the wall
            c2ws[srcs[1], :3, 3] = c2ws[ref, :3, 3] + c2ws[ref, :3, :3] @ np.array([0.02, 0.01, 1.4])
    elif pose == "rotated":
        c2ws[ref] = c2ws[ref] @ _rot("z", 0.5) @ _rot("y", 0.12)
    elif pose != "scene":
        raise ValueError(pose)
    win["c2ws"] = c2ws.astype(np.float32)
    win["depth_min"], win["depth_max"] = dmin, dmax
    return win


# the windows the E_* constants are the maximum over, and the sensitivity test runs on: (height, width, views, pose)
# (the oracle's coordinate rounding grows with the coordinate: the largest shape of the GPU test is among them)
CPU_WINDOWS = ((64, 96, 4, "scene"), (64, 96, 3, "narrow"), (64, 96, 4, "behind"), (64, 96, 3, "rotated"), (96, 64, 2, "scene"),
               (96, 160, 4, "rotated"))
# the smallest windows the engine accepts (any positive multiple of 32) and the model each runs with in the CPU tests: stage 1 is an 8 x 8 map
# whose CostRegNet bottoms out at (6, 1, 1); at 48/4/4 stage 3 bottoms out at ONE plane, (1, 4, 4).  Not part of the maxima E_VOL .. E_FEAT record.
SMALL_WINDOWS = ((32, 32, 2, "scene"), (32, 32, 4, "behind"), (32, 64, 3, "rotated"), (64, 32, 8, "narrow"), (32, 96, 3, "rotated"),
                 (96, 32, 2, "behind"))
SMALL_MODELS = ("trained", (48, 4, 4), (16, 8, 8), "trained", (48, 4, 4), "trained")


def model_order(views, ref_index):
    return [ref_index] + [i for i in range(views) if i != ref_index]


def stage_K(K, stage):
    """Rows 0-1 of the full-resolution K times 0.25 / 0.5 / 1, the product taken in double and stored as float."""
    k = np.asarray(K, np.float32).reshape(3, 3).astype(np.float64)
    k[:2] = (np.float64((0.25, 0.5, 1.0)[stage - 1]) * k[:2]).astype(np.float32)
    return k


def gate_weights(tensors, stage):
    p = "volume_gates.stage%d." % stage
    return {k[len(p):]: np.asarray(v, np.float64) for k, v in tensors.items() if k.startswith(p)}


# ------------------------------------------------------------------ hypothesis planes
def _up2(prev, h, w):
    """x2 bilinear upsampling, align_corners=False: src = max(0.5 (dst + 0.5) - 0.5, 0), the far tap clamped to the last row / column."""
    prev = np.asarray(prev, np.float64)
    hp, wp = prev.shape
    assert (h, w) == (2 * hp, 2 * wp)
    sy = np.maximum(0.5 * (np.arange(h) + 0.5) - 0.5, 0.0)
    sx = np.maximum(0.5 * (np.arange(w) + 0.5) - 0.5, 0.0)
    y0, x0 = np.floor(sy).astype(int), np.floor(sx).astype(int)
    y1, x1 = np.minimum(y0 + 1, hp - 1), np.minimum(x0 + 1, wp - 1)
    ly, lx = (sy - y0)[:, None], (sx - x0)[None, :]
    top = (1 - lx) * prev[y0][:, x0] + lx * prev[y0][:, x1]
    bot = (1 - lx) * prev[y1][:, x0] + lx * prev[y1][:, x1]
    return (1 - ly) * top + ly * bot


def planes64(stage, engine_prev_depth, dmin, dmax, meta, h, w):
    """(D, h, w) hypothesis depths.  Stage 1: D uniform planes dmin .. dmax.  Later stages: around the x2 upsampled previous-stage
    depth (the caller passes the ENGINE's), lo = max(cur - D/2 Delta, 1e-3), d_k = lo + (hi - lo) k / D with hi = lo + D Delta and
    Delta = interval_ratio[stage] * (dmax - dmin) / (D_1 - 1).  dmin, dmax are the float values the operator receives."""
    dmin, dmax = float(np.float32(dmin)), float(np.float32(dmax))
    D = int(meta["depth_num"][stage - 1])
    base = (dmax - dmin) / (int(meta["depth_num"][0]) - 1)
    k = np.arange(D, dtype=np.float64).reshape(D, 1, 1)
    if stage == 1:
        return np.broadcast_to(dmin + base * k, (D, h, w)).copy()
    delta = float(np.float32(meta["interval_ratio"][stage - 1])) * base
    return adaptive_planes64(engine_prev_depth, D, delta, h, w)


def adaptive_planes64(prev, D, delta, h, w, mutant=None):
    """(D, h, w) planes around the x2 upsampled `prev` (h / 2, w / 2): lo = max(cur - D/2 delta, 1e-3), d_k = lo + (hi - lo) k / D, hi = lo + D delta.
    The kernels' PlaneArgs in double: half_range = D/2 delta, full_range = D delta.  mutant "no_lo_clamp": the 1e-3 clamp left out."""
    assert mutant in (None, "no_lo_clamp"), mutant
    k = np.arange(D, dtype=np.float64).reshape(D, 1, 1)
    cur = _up2(prev, h, w)
    lo = cur - (D / 2.0) * delta
    if mutant is None:
        lo = np.maximum(lo, 1e-3)
    hi = lo + D * delta
    return lo[None] + (hi - lo)[None] * (k / D)


def uniform_planes64(dmin, interval, D, h, w):
    """(D, h, w) planes dmin + interval k (PlaneArgs with prev == NULL), from the float values the kernel receives."""
    k = np.arange(D, dtype=np.float64).reshape(D, 1, 1)
    return np.broadcast_to(float(np.float32(dmin)) + float(np.float32(interval)) * k, (D, h, w)).copy()


# ------------------------------------------------------------------ cost volume
def _inv_h(c2w):
    return np.linalg.inv(np.asarray(c2w, np.float64).reshape(4, 4))


def homography(K_stage, c2w_ref, c2w_src):
    """Reference pixel (x, y, 1) * depth -> source pixel: M = [K w2c_src] [K w2c_ref]^-1, every inverse in double."""
    K = np.asarray(K_stage, np.float64).reshape(3, 3)

    def w2p(c2w):
        m = _inv_h(c2w)
        m[:3, :4] = K @ m[:3, :4]
        return m
    return w2p(c2w_src) @ np.linalg.inv(w2p(c2w_ref))


def _bn1(x, g, p):
    return (x - g[p + ".running_mean"][0]) / np.sqrt(g[p + ".running_var"][0] + BN_EPS) * g[p + ".weight"][0] + g[p + ".bias"][0]


def cost_volume64(feats, planes, K_stage, c2w, gate_w, view_aggregation, nsrc_divisor=None, mutant=None, return_stats=False):
    """feats (V, h, w, C), planes (D, h, w), c2w (V, 4, 4) in model order -> volume (D, h, w, C).
    A source sample is valid iff pz >= 0.001 and -1 < u < w and -1 < v < h; it is the bilinear mix of its four taps read from the
    source map with a one-pixel zero border, else 0.  View aggregation: mean over the sources of (g + 1) d^2 with d = warped - ref
    and g = relu(BN(conv1x1(relu(BN(conv1x1(d^2))))))); otherwise the variance over all views, s2 / V - (s / V)^2.
    nsrc_divisor: the divisor of the mean where it is not V - 1 (a view shard).
    mutant: one of MUTANTS, a deliberate one-line mistake (tests/test_mvs_stage_ref.py shows each moves the volume beyond the bound
    the GPU test sets); `spacing_Dm1` re-spaces the given planes from k / D to k / (D - 1) about plane 0.
    return_stats: also dict(behind=share of samples with pz < 0.001, outside=share of the others outside the source image)."""
    assert mutant is None or mutant in MUTANTS, mutant
    feats = np.asarray(feats, np.float64)
    planes = np.asarray(planes, np.float64)
    V, h, w, C = feats.shape
    D = planes.shape[0]
    if mutant == "spacing_Dm1":
        k = np.arange(D, dtype=np.float64).reshape(D, 1, 1)
        planes = planes[0][None] + (planes[1] - planes[0])[None] * D * (k / (D - 1))
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    ref = feats[0][None]  # (1, h, w, C)
    nsrc = V - 1
    last = nsrc - 1 if mutant == "drop_last_view" else nsrc
    acc = np.zeros((D, h, w, C))
    s1 = np.broadcast_to(ref, (D, h, w, C)).copy()
    s2 = s1 ** 2
    n_behind = n_outside = 0
    for v in range(1, 1 + last):
        M = homography(K_stage, c2w[0], c2w[v])
        rx = M[0, 0] * xs + M[0, 1] * ys + M[0, 2]
        ry = M[1, 0] * xs + M[1, 1] * ys + M[1, 2]
        rz = M[2, 0] * xs + M[2, 1] * ys + M[2, 2]
        px, py, pz = rx[None] * planes + M[0, 3], ry[None] * planes + M[1, 3], rz[None] * planes + M[2, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            u, vv = px / pz, py / pz
        if mutant == "shift":
            u = u + 1e-3
        front = pz >= 0.001
        if mutant == "border":
            inside = (u >= 0) & (u <= w - 1) & (vv >= 0) & (vv <= h - 1)
        else:
            inside = (u > -1) & (u < w) & (vv > -1) & (vv < h)  # (NaN fails)
        valid = inside if mutant == "no_behind_mask" else (front & inside)
        n_behind += int((~front).sum())
        n_outside += int((front & ~inside).sum())
        uc, vc = np.where(valid, u, -1.0), np.where(valid, vv, -1.0)
        x0, y0 = np.floor(uc), np.floor(vc)
        ax, ay = (uc - x0)[..., None], (vc - y0)[..., None]
        xi, yi = x0.astype(np.int64) + 1, y0.astype(np.int64) + 1  # indices into the bordered map: 0 .. w, 0 .. h
        src = np.zeros((h + 2, w + 2, C))
        src[1:-1, 1:-1] = feats[v]
        warped = ((1 - ax) * (1 - ay) * src[yi, xi] + ax * (1 - ay) * src[yi, xi + 1] +
                  (1 - ax) * ay * src[yi + 1, xi] + ax * ay * src[yi + 1, xi + 1]) * valid[..., None]
        if view_aggregation:
            d2 = (warped - ref) ** 2
            if mutant == "no_gate":
                g = 0.0
            else:
                z = d2 @ gate_w["0.weight"].reshape(C) + gate_w["0.bias"][0]
                z = np.maximum(_bn1(z, gate_w, "1"), 0.0)
                z = z * gate_w["3.weight"].reshape(()) + gate_w["3.bias"][0]
                g = np.maximum(_bn1(z, gate_w, "4"), 0.0)[..., None]
            acc += (g + 1.0) * d2
        else:
            s1 += warped
            s2 += warped ** 2
    if view_aggregation:
        div = float(nsrc_divisor if nsrc_divisor is not None else nsrc)
        vol = acc / (div + 1.0 if mutant == "divisor_V" else div)
    else:
        n = float(V + 1 if mutant == "divisor_V" else V)
        vol = s2 / n - (s1 / n) ** 2
    if return_stats:
        total = float(max(last, 1) * D * h * w)
        return vol, dict(behind=n_behind / total, outside=n_outside / total)
    return vol


# ------------------------------------------------------------------ prob head, regression, FeatureNet
def prob64(x11, prob_weight):
    """x11 (D, h, w, 8), weight (1, 8, 3, 3, 3) -> logits (D, h, w): conv3d, padding 1."""
    x = torch.from_numpy(np.ascontiguousarray(np.asarray(x11, np.float64))).permute(3, 0, 1, 2)[None]
    wt = torch.from_numpy(np.asarray(prob_weight, np.float64))
    return F.conv3d(x, wt, None, 1, 1)[0, 0].numpy()


def regress64(logits, planes):
    """Returns (depth (h, w), E[k] (h, w), sum4 (D, h, w)): softmax over D, its expectation over the planes and over the plane index,
    and sum4[i] = p[i-1] + p[i] + p[i+1] + p[i+2] (planes outside 0 .. D-1 count 0): the confidence is sum4 at i = clamp(trunc(E[k]))."""
    lg = np.asarray(logits, np.float64)
    D = lg.shape[0]
    e = np.exp(lg - lg.max(axis=0, keepdims=True))
    p = e / e.sum(axis=0, keepdims=True)
    depth = (p * np.asarray(planes, np.float64)).sum(axis=0)
    ek = (p * np.arange(D, dtype=np.float64).reshape(D, 1, 1)).sum(axis=0)
    pp = np.concatenate([np.zeros((1,) + p.shape[1:]), p, np.zeros((2,) + p.shape[1:])])
    sum4 = pp[0:D] + pp[1:D + 1] + pp[2:D + 2] + pp[3:D + 3]
    return depth, ek, sum4


# deliberate one-line mistakes of the REGRESSION (tests/test_mvs_adversarial_ref.py shows each leaves the bound of, or breaks an exact comparison of,
# tests/test_mvs_adversarial_gpu.py on that test's own inputs):
#   no_max_subtraction   softmax as exp(x) / sum exp(x)
#   rint                 the confidence window around rint(E[k]) instead of trunc(E[k])
#   window_m1_p1         the window idx-1 .. idx+1
#   window_m2_p1         the window idx-2 .. idx+1
#   no_idx_clamp         index and window taken without the clamp to 0 .. D-1: a tap outside the range reads the plane modulo D instead of counting 0.
#                        (The clamp of trunc(E[k]) ALONE cannot be reached by finite logits -- E[k] is a convex combination of 0 .. D-1, and the few ulps by
#                        which an fp32 sum may exceed D-1 do not survive the truncation -- so the mutant removes it together with the range test of the taps.)
# and of the PLANES: adaptive_planes64(mutant="no_lo_clamp").
REGRESS_MUTANTS = ("no_max_subtraction", "rint", "window_m1_p1", "window_m2_p1", "no_idx_clamp")


def regress_out64(logits, planes, mutant=None):
    """(depth, conf) of regress64 with the confidence gathered at clamp(trunc(E[k])); mutant: one of REGRESS_MUTANTS."""
    assert mutant is None or mutant in REGRESS_MUTANTS, mutant
    lg = np.asarray(logits, np.float64)
    D = lg.shape[0]
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(lg if mutant == "no_max_subtraction" else lg - lg.max(axis=0, keepdims=True))
        p = e / e.sum(axis=0, keepdims=True)
    depth = (p * np.asarray(planes, np.float64)).sum(axis=0)
    ek = (p * np.arange(D, dtype=np.float64).reshape(D, 1, 1)).sum(axis=0)
    with np.errstate(invalid="ignore"):
        idx = np.nan_to_num(np.rint(ek) if mutant == "rint" else np.trunc(ek)).astype(np.int64)
    lo, hi = {"window_m1_p1": (-1, 1), "window_m2_p1": (-2, 1)}.get(mutant, (-1, 2))
    conf = np.zeros(ek.shape)
    for o in range(lo, hi + 1):
        k = idx + o
        if mutant == "no_idx_clamp":
            conf += np.take_along_axis(p, (k % D)[None], axis=0)[0]
        else:
            k0 = np.clip(idx, 0, D - 1) + o
            conf += np.where((k0 >= 0) & (k0 < D), np.take_along_axis(p, np.clip(k0, 0, D - 1)[None], axis=0)[0], 0.0)
    return depth, conf


def conf_at(sum4, idx):
    D = sum4.shape[0]
    return np.take_along_axis(sum4, np.clip(idx, 0, D - 1)[None].astype(np.int64), axis=0)[0]


def conf_error(conf, ek, sum4):
    """|conf - sum4[trunc(E[k])]| per pixel; where E[k] lies within EK_INTEGER_BAND of an integer r, the smaller of the errors at r - 1 and r."""
    r = np.rint(ek)
    near = np.abs(ek - r) <= EK_INTEGER_BAND
    err = np.abs(conf - conf_at(sum4, np.trunc(ek)))
    alt = np.minimum(np.abs(conf - conf_at(sum4, r - 1)), np.abs(conf - conf_at(sum4, r)))
    return np.where(near, np.minimum(err, alt), err), near


class _W64:
    def __init__(self, tensors):
        self.t = {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in tensors.items() if k.startswith("feature_net.")}

    def __getitem__(self, k):
        return self.t[k]


def features64(bgrs, tensors, ref_index=0):
    """The oracle's preprocess + feature_net with double weights and a double image (the u8 -> float image itself is the input: its
    float values, exactly).  Returns [feat1, feat2, feat3], each (V, h, w, C) in model order."""
    from oracle import mvsnet_oracle as O
    K = np.eye(3, dtype=np.float32)
    image, _, _ = O.preprocess(bgrs, K, [np.eye(4, dtype=np.float32)] * len(bgrs), ref_index)
    with torch.no_grad():
        feats = O.feature_net(image.double(), _W64(tensors))
    return [f.permute(0, 2, 3, 1).contiguous().numpy() for f in feats]


def rng_of(x):
    return float(np.max(x) - np.min(x))


def border_slices():
    """The four image borders of a (D, h, w, ...) tensor, named."""
    return (("row 0", np.s_[:, 0]), ("row h-1", np.s_[:, -1]), ("column 0", np.s_[:, :, 0]), ("column w-1", np.s_[:, :, -1]))


# ------------------------------------------------------------------ layer restatements (CostRegNet, FeatureNet)
# deliberate one-line mistakes of a LAYER (tests/test_mvs_stage_ref.py shows each moves some layer of some small window beyond 20 x the bound):
#   skip_before_relu   relu(bn + skip) where the network computes relu(bn) + skip
#   deconv_phase       a transposed layer's output padding placed at the front: the odd and the even output phases swap
#   replicate_border   the zero padding replaced by the edge value
#   stride_phase       a strided layer sampling the odd positions
LAYER_MUTANTS = ("skip_before_relu", "deconv_phase", "replicate_border", "stride_phase")


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def _tup(v, nd):
    return (int(v),) * nd if np.isscalar(v) else tuple(int(i) for i in v)


def _bn64(y, tensors, prefix):
    """Eval-mode BatchNorm over the last (channel) axis: (y - mean) / sqrt(var + eps) * weight + bias."""
    mean, var, g, b = (_t64(tensors[prefix + "." + n]) for n in ("running_mean", "running_var", "weight", "bias"))
    return (y - mean) / torch.sqrt(var + BN_EPS) * g + b


def _conv64(x, weight, stride=1, bias=None, mutant=None):
    """x channels-last, (D, h, w, Cin) for a 5-D weight and (V, h, w, Cin) for a 4-D one; padding k // 2, written out as an explicit border
    around the input.  Returns channels-last float64 (torch)."""
    w = _t64(weight)
    nd = w.dim() - 2
    x = _t64(x)
    x = x.permute(3, 0, 1, 2)[None] if nd == 3 else x.permute(0, 3, 1, 2)
    stride = _tup(stride, nd)
    pads = []
    for k in reversed(w.shape[2:]):
        pads += [k // 2, k // 2]
    if any(pads):
        x = F.pad(x, pads, mode="replicate" if mutant == "replicate_border" else "constant")
    if mutant == "stride_phase":
        for ax, s in enumerate(stride):
            n = x.shape[2 + ax] - 2 * (w.shape[2 + ax] // 2)
            if s > 1 and n % s == 0:  # (an axis of one position has no odd position to sample)
                x = x.narrow(2 + ax, 1, x.shape[2 + ax] - 1)
    y = (F.conv3d if nd == 3 else F.conv2d)(x, w, None if bias is None else _t64(bias), stride, 0)
    return y[0].permute(1, 2, 3, 0) if nd == 3 else y.permute(0, 2, 3, 1)


def layer_scale(out, pre):
    """The unit of a layer's error: max(max |value before the ReLU|, max |output|) of the float64 layer."""
    return float(max(np.abs(pre).max(), np.abs(out).max()))


def conv_bn_relu64(x, tensors, prefix, stride, mutant=None):
    """Conv (no bias, padding k // 2: 1 for CostRegNet's Conv3d) + BatchNorm (eval, eps 1e-5) + ReLU.  x (D, h, w, Cin) with a 5-D weight, (V, h, w, Cin) with
    a 4-D one.  Returns (output, value before the ReLU), float64 numpy."""
    assert mutant is None or mutant in LAYER_MUTANTS, mutant
    pre = _bn64(_conv64(x, tensors[prefix + ".conv.weight"], stride, None, mutant), tensors, prefix + ".bn")
    return torch.relu(pre).numpy(), pre.numpy()


def deconv_bn_relu_skip64(x, skip, tensors, prefix, stride, output_padding, mutant=None):
    """ConvTranspose3d (k 3, padding 1) + BatchNorm + ReLU, THEN + skip.  The transposed convolution is written as: zeros inserted between the input
    positions along the strided axes, a border of k - 1 - padding = 1 in front and 1 + output_padding behind, and a plain convolution with the kernel
    flipped and its channel axes exchanged.  x (D, h, w, Cin), skip (D', h', w', Cout).  Returns (output, value before the ReLU)."""
    assert mutant is None or mutant in LAYER_MUTANTS, mutant
    w = _t64(tensors[prefix + ".conv.weight"])  # (Cin, Cout, 3, 3, 3)
    assert tuple(w.shape[2:]) == (3, 3, 3)
    x = _t64(x)
    (sd, sh, sw), opad = _tup(stride, 3), _tup(output_padding, 3)
    D, h, w_, C = x.shape
    z = torch.zeros(((D - 1) * sd + 1, (h - 1) * sh + 1, (w_ - 1) * sw + 1, C), dtype=torch.float64)
    z[::sd, ::sh, ::sw] = x
    pads = []
    for op in reversed(opad):
        pads += [1 + op, 1] if mutant == "deconv_phase" else [1, 1 + op]
    z = F.pad(z.permute(3, 0, 1, 2)[None], pads, mode="replicate" if mutant == "replicate_border" else "constant")
    y = F.conv3d(z, w.flip(2, 3, 4).transpose(0, 1).contiguous())[0].permute(1, 2, 3, 0)
    pre = _bn64(y, tensors, prefix + ".bn")
    skip = _t64(skip)
    assert skip.shape == pre.shape, (tuple(skip.shape), tuple(pre.shape))
    out = torch.relu(pre + skip) if mutant == "skip_before_relu" else torch.relu(pre) + skip
    return out.numpy(), pre.numpy()


def image64(bgrs, ref_index):
    """(V, H, W, 3) RGB in model order: the float values of u8 / 255 (the quotient taken in double, stored as float), exactly."""
    order = model_order(len(bgrs), ref_index)
    return np.stack([(np.asarray(bgrs[v])[..., ::-1].astype(np.float64) / 255.0).astype(np.float32).astype(np.float64) for v in order])


def _up2_nearest(x):
    return np.repeat(np.repeat(np.asarray(x, np.float64), 2, axis=1), 2, axis=2)


_FN = "feature_net."


def fn_conv0_1_64(image, tensors, mutant=None):
    """fn.conv0.1 from the image: conv0.0 and conv0.1, both 3 x 3 + BN + ReLU (the engine's k_fn_front leaves no fn.conv0.0)."""
    a, _ = conv_bn_relu64(image, tensors, _FN + "conv0.0", 1, mutant)
    return conv_bn_relu64(a, tensors, _FN + "conv0.1", 1, mutant)


def fn_cbr64(name):
    """fn.conv1.0 .. fn.conv2.2 from the tensor before it: conv{1,2}.0 are 5 x 5 with stride 2, the others 3 x 3."""
    stride = 2 if name.endswith(".0") else 1
    return lambda x, tensors, mutant=None: conv_bn_relu64(x, tensors, _FN + name[len("fn."):], (stride, stride), mutant)


def fn_feat1_64(c1, tensors, mutant=None):
    """feat1 from fn.conv2.2: out.stage1, 1 x 1, no bias (no ReLU: the value `before` it is the output)."""
    y = _conv64(c1, tensors[_FN + "out.stage1.weight"], 1, None, mutant).numpy()
    return y, y


def fn_inter2_64(c2, c1, tensors, mutant=None):
    """inter2 from fn.conv1.2 and fn.conv2.2: the nearest x2 upsampling of conv2.2 + skip.stage2 (1 x 1, bias) of conv1.2."""
    y = _up2_nearest(c1) + _conv64(c2, tensors[_FN + "skip.stage2.weight"], 1, tensors[_FN + "skip.stage2.bias"], mutant).numpy()
    return y, y


def fn_feat2_64(i2, tensors, mutant=None):
    """feat2 from inter2: out.stage2, 3 x 3, no bias."""
    y = _conv64(i2, tensors[_FN + "out.stage2.weight"], 1, None, mutant).numpy()
    return y, y


def fn_feat3_64(c3, i2, tensors, mutant=None):
    """feat3 from fn.conv0.1 and inter2, in the literal order: inter3 = up(inter2) + skip.stage3 (1 x 1, bias) of conv0.1, then out.stage3 (3 x 3, no bias)."""
    i3 = _up2_nearest(i2) + _conv64(c3, tensors[_FN + "skip.stage3.weight"], 1, tensors[_FN + "skip.stage3.bias"], mutant).numpy()
    y = _conv64(i3, tensors[_FN + "out.stage3.weight"], 1, None, mutant).numpy()
    return y, y


class Layer:
    """One engine tensor and the float64 statement of the layer(s) that produce it: fn(*inputs, tensors, mutant=) -> (output, value before the ReLU).
    inputs: engine tensor names ("images": the window's u8 images, passed as image64)."""

    def __init__(self, name, inputs, fn, strided=False, transposed=False):
        self.name, self.inputs, self.fn, self.strided, self.transposed = name, tuple(inputs), fn, strided, transposed

    def mutants(self):
        return ("replicate_border",) + (("stride_phase",) if self.strided else ()) + (("deconv_phase", "skip_before_relu") if self.transposed else ())


def feature_net_layers():
    L = [Layer("fn.conv0.1", ("images",), fn_conv0_1_64)]
    prev = "fn.conv0.1"
    for n in ("fn.conv1.0", "fn.conv1.1", "fn.conv1.2", "fn.conv2.0", "fn.conv2.1", "fn.conv2.2"):
        L.append(Layer(n, (prev,), fn_cbr64(n), strided=n.endswith(".0")))
        prev = n
    L += [Layer("feat1", ("fn.conv2.2",), fn_feat1_64), Layer("inter2", ("fn.conv1.2", "fn.conv2.2"), fn_inter2_64),
          Layer("feat2", ("inter2",), fn_feat2_64), Layer("feat3", ("fn.conv0.1", "inter2"), fn_feat3_64)]
    return L


def cost_reg_layers(stage, D):
    """CostRegNet of one stage as the engine names it: s{S}.conv0 .. conv6, the transposed conv7 / conv9 / conv11 with their skips conv4 / conv2 / conv0.
    With D = 4 planes conv5 and conv7 keep the depth axis: stride (1, 2, 2), conv7's output padding (0, 1, 1)."""
    s, p = "s%d." % stage, "cost_regularization_net.stage%d." % stage
    s5, op7 = ((1, 2, 2), (0, 1, 1)) if D == 4 else ((2, 2, 2), (1, 1, 1))

    def cbr(n, stride):
        return lambda x, tensors, mutant=None: conv_bn_relu64(x, tensors, p + n, stride, mutant)

    def dbr(n, stride, opad):
        return lambda x, skip, tensors, mutant=None: deconv_bn_relu_skip64(x, skip, tensors, p + n, stride, opad, mutant)

    L, prev = [], "volume%d" % stage
    for n, stride in (("conv0", 1), ("conv1", 2), ("conv2", 1), ("conv3", 2), ("conv4", 1), ("conv5", s5), ("conv6", 1)):
        L.append(Layer(s + n, (prev,), cbr(n, _tup(stride, 3)), strided=stride != 1))
        prev = s + n
    for n, skip, stride, opad in (("conv7", "conv4", s5, op7), ("conv9", "conv2", (2, 2, 2), (1, 1, 1)), ("conv11", "conv0", (2, 2, 2), (1, 1, 1))):
        L.append(Layer(s + n, (prev, s + skip), dbr(n, stride, opad), transposed=True))
        prev = s + n
    return L


def all_layers(meta):
    """Every layer between the images and the three x11 tensors, in execution order."""
    L = feature_net_layers()
    for s in (1, 2, 3):
        L += cost_reg_layers(s, int(meta["depth_num"][s - 1]))
    return L
