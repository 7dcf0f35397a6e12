// mvs_plan.h -- the launch plan of one DrMvsnet window shape (H, W, V) as a value (included by dr_mvsnet.hip only).
//   Op / launch_op / op_kernel_name : one launch of the plan with its typed arguments; the ONE switch over the op kinds; the ONE place that names an op's kernel
//   MvsPlan        : everything that lives exactly as long as a window shape -- the named device tensors, the constants, the image / select / cache-entry
//                    buffers, the pinned input and result blocks -- and what was built over them (op lists, fork range, per-stage arguments).  Its destructor
//                    releases all of it; a plan that fails half way through its construction leaves nothing behind.
//   MvsPlanBuilder : which layers exist (cva_mvsnet.py:98-184, module.py:461-531), from the weights, the switches and the window shape
// What changes per call (cameras, plane ranges, the filter's rank: WindowArgs) and the control flow of a forward stay in the engine.
#pragma once
#include <memory>

#include "conv_mfma.h"
#include "mvs_host.h"
#include "mvs_launch.h"
#ifdef DR_PARITY_HOOKS  // conv11 + prob in one launch: built twice in round 5, correct, slower than the two-kernel path (profiles/r05_tail.txt): parity build only
#include "tail_kernels.h"
#endif
#include "fn_front.h"
#include "fn_head3.h"
#include "hip_owner.h"

namespace dr {

#ifdef DR_PARITY_HOOKS
constexpr bool kParityHooks = true;
#else
constexpr bool kParityHooks = false;
#endif

struct DevTensor {
  float *d = nullptr;
  int D = 0, H = 0, W = 0, C = 0;
  int pad = 0;  // zero border (pixels) around every H x W plane in memory; H and W stay the logical size
  int split = 0;  // 16: stored as C / 16 consecutive (D,H,W,16) sub-tensors (stage 1's cost volume: each 16-channel pass of conv0 then reads whole records)
  size_t n() const { return (size_t)D * (H + 2 * pad) * (W + 2 * pad) * C; }         // floats in memory
  float *interior() const { return d + ((size_t)pad * (W + 2 * pad) + pad) * C; }    // first logical pixel
};

struct Op {
  enum Kind { PREPROCESS, CONV, SKIPUP, PROB, COSTVOL, REGRESS, EDGE, HIST, SCAN, APPLY, BORDERFIX, TAIL, FRONT, HEAD3 } kind;
  std::string name;
  int stage = 0;                          // COSTVOL, PROB, TAIL, REGRESS: the network stage 1..3 (their arguments are per stage: MvsPlan::pr, WindowArgs)
  int level = 0;                          // HIST, SCAN: the level 0..2 of the edge filter's select (EDGE, HIST, SCAN, APPLY share MvsPlan::filt)
  ConvLaunch conv;                        // CONV only
#ifdef DR_PARITY_HOOKS
  TailArgs tail{};                        // TAIL only: conv11 + prob in one launch (tail_kernels.h)
#endif
  FrontArgs front{};                      // FRONT only: preprocess + conv0.0 + conv0.1 in one launch (fn_front.h)
  Head3Args head3{};                      // HEAD3 only: FeatureNet's folded stage-3 head in one launch (fn_head3.h)
  PreprocessArgs pre{};                   // PREPROCESS only
  SkipUpArgs skip{};                      // SKIPUP only
  BorderFixArgs border{};                 // BORDERFIX only
  std::function<ConvLaunch(int)> replan;  // CONV only: build candidate `rank` of the planner's ranking
  std::string sig;                        // CONV only: layer signature in conv_tuned.h's column order
  int ncand = 0;
  double flops = 0, bytes = 0;
};

// FeatureNet for a batch of views: its launches, and which of them may run on the side stream
struct FeatureNetOps {
  std::vector<Op> ops;
  size_t fork_lo = 0, fork_hi = 0, feat2_op = 0;  // ops [fork_lo, fork_hi) = fn.skip2 .. fn.out3; feat2_op: the one that completes feat2
};
struct FnOut { size_t op; int stage; size_t offset; };  // launch `op` of the single-view plan stores into feat<stage + 1> at this float offset
struct FcBuffers { float *feat[3] = {nullptr, nullptr, nullptr}; uint8_t *bgr = nullptr; };  // entry e of the feature cache's index (mvs_host.h): its three bordered feature maps and its image

// what a call derives from its cameras and ranges (WindowStager::fill_args, mvs_stage.h): the plan's launches read it next to their own arguments
struct WindowArgs {
  CostVolArgs cv[3];
  RegressArgs rg[3];
  unsigned filter_rank = 0;
};

inline bool same_instance(const ConvLaunch &a, const ConvLaunch &b) {
  return a.async == b.async && a.ci == b.ci && a.ct == b.ct && a.pt == b.pt && a.fz == b.fz && a.bf3 == b.bf3 && a.nup == b.nup && a.ncw == b.ncw &&
         a.march.wino == b.march.wino && a.march.rm == b.march.rm;
}

struct MvsPlan {  // (not copyable: its owner is not)
  DevTensor &T(const std::string &name) {
    auto it = tensors.find(name);
    if (it == tensors.end()) fail(DR_ERR_ARG, "unknown tensor '%s'", name.c_str());
    return it->second;
  }
  // every launch of the single-view plan becomes the batch plan's own kernel instance for that layer (the planner ranks candidates by a cost model that sees
  // the batch size; the arithmetic of an instance does not)
  bool match_fn1() {
    for (Op &o : ops1) {
      const Op *b = nullptr;
      for (size_t i = 0; i < fork_hi && i < ops.size(); ++i) if (ops[i].name == o.name) b = &ops[i];
      if (!b || b->kind != o.kind) return false;
      if (o.kind == Op::FRONT || o.kind == Op::HEAD3) continue;
      if (o.kind != Op::CONV) return false;
      for (int r = 0; r < o.ncand && !same_instance(o.conv, b->conv); ++r) o.conv = o.replan(r);  // (ncand > 0 only with a replan; no match: the caller drops ops1)
      if (!same_instance(o.conv, b->conv)) return false;
    }
    return true;
  }

  HipOwner own;       // the tensors, the image / select / cache-entry buffers, the pinned blocks
  DeviceArena arena;  // the constants: weights, tap tables (the ops' replan closures plan into it: a plan lives at one address)
  std::map<std::string, DevTensor> tensors;
  std::vector<Op> ops;
  size_t fork_lo = 0, fork_hi = 0, feat2_op = 0;  // FeatureNetOps' of the batch plan
  ProbArgs pr[3] = {};  // per stage; x == nullptr where the plan has no PROB op
  FilterArgs filt{};
  uint8_t *d_bgr = nullptr, *h_in = nullptr;  // the window's images on the device, and the pinned block they are gathered in
  float *h_out[2] = {nullptr, nullptr}, *h_out_dev[2] = {nullptr, nullptr};  // two pinned result blocks (4 maps each), used alternately, and the addresses the device uses for them
  // key-frame feature cache (FeatureCacheDev, mvs_cache.h): FeatureNet for ONE view, where its three outputs go, the entries.  ops1 is empty where the
  // window shape, the switches or the planner's candidates do not allow it.
  std::vector<Op> ops1;
  std::vector<FnOut> fn1_out;
  std::vector<FcBuffers> fcache;
};

// The one switch over the op kinds.  (A view-shard's collectives around COSTVOL and REGRESS are the caller's: MvsEngine::forward.)
inline void launch_op(const Op &o, const MvsPlan &p, const WindowArgs &w, const MvsSwitches &sw, hipStream_t st) {
  switch (o.kind) {
    case Op::PREPROCESS: launch_preprocess(o.pre, st); break;
    case Op::CONV: launch_conv(o.conv, st); break;
    case Op::BORDERFIX: launch_out3_border(o.border, st); break;
    case Op::SKIPUP: launch_skip_up(o.skip, st); break;
    case Op::PROB: launch_prob(p.pr[o.stage - 1], w.rg[o.stage - 1], sw, o.stage, st); break;
    case Op::TAIL:
#ifdef DR_PARITY_HOOKS
      launch_tail(o.tail, st);
#endif  // (the product plans no TAIL op)
      break;
    case Op::FRONT: launch_fn_front(o.front, st); break;
    case Op::HEAD3: launch_fn_head3(o.head3, st); break;
    case Op::COSTVOL: launch_costvol(w.cv[o.stage - 1], sw, o.stage, st); break;
    case Op::REGRESS: {
      // (where the stage's PROB op ran k_prob2_regress, the regression is done: the same choice function says so here and there)
      const ProbArgs &pr = p.pr[o.stage - 1];
      if (!(pr.x && choose_prob(prob_shape(pr), sw, o.stage).regresses())) launch_regress(w.rg[o.stage - 1], sw, st);
      break;
    }
    case Op::EDGE: launch_edge(p.filt, w.filter_rank, st); break;
    case Op::HIST: launch_hist(p.filt, o.level, st); break;
    case Op::SCAN: launch_scan(p.filt, o.level, st); break;
    case Op::APPLY: launch_apply(p.filt, st); break;
  }
}

// the kernel instance launch_op runs for `o`, as drm_profile prints it
inline void op_kernel_name(const Op &o, const MvsPlan &p, const WindowArgs &w, const MvsSwitches &sw, char *kn, size_t cap) {
  if (o.kind == Op::CONV) conv_instance_name(o.conv, kn, cap);
  else if (o.kind == Op::COSTVOL) choose_costvol(costvol_shape(w.cv[o.stage - 1]), sw, o.stage).name(kn, cap);
  else if (o.kind == Op::PROB) choose_prob(prob_shape(p.pr[o.stage - 1]), sw, o.stage).name(kn, cap);
#ifdef DR_PARITY_HOOKS
  else if (o.kind == Op::TAIL) snprintf(kn, cap, o.tail.wmf ? "k_tail_m<%d>" : "k_tail<%d>", std::max(3, tail_nout(o.tail.QY, o.tail.QX)));
#endif
  else if (o.kind == Op::REGRESS) snprintf(kn, cap, "k_regress");
  else if (o.kind == Op::PREPROCESS) snprintf(kn, cap, "k_preprocess");
  else if (o.kind == Op::FRONT) snprintf(kn, cap, "k_fn_front");
  else if (o.kind == Op::HEAD3) snprintf(kn, cap, "k_fn_head3");
  else if (o.kind == Op::SKIPUP) snprintf(kn, cap, "k_skip_up<%d>", o.skip.cin);
  else if (o.kind == Op::BORDERFIX) snprintf(kn, cap, "k_out3_border");
  else snprintf(kn, cap, "k_filter");
}

// ------------------------------------------------------------------ construction
// MvsPlanBuilder{what it reads}.build(): the whole plan for one window shape.  A throw (out of memory, unsupported depth_num, missing tensor) leaves nothing
// allocated.  The plan keeps lut and march_err, the engine's, which outlive it.
struct MvsPlanBuilder {
  const Blob &blob_;
  const MvsSwitches &sw_;
  int device_;
  const float *lut_;  // u8 -> [0, 1] table on the device
  int *march_err_;    // pinned, device-visible: k_conv_m raises it when a ring wait gives up
  int H, W, V;
  int shard_nsrc_;    // > 0: a view-shard rank (no feature cache)
  int fcache_cap_;    // entries of the key-frame feature cache (0: off)
  std::unique_ptr<MvsPlan> plan_ = std::make_unique<MvsPlan>();
  MvsPlan &p_ = *plan_;

  std::unique_ptr<MvsPlan> build() {
    p_.arena.err_flag = march_err_;
    for (int b = 0; b < 2; ++b) p_.h_out[b] = p_.own.pinned<float>((size_t)H * W * 4, &p_.h_out_dev[b]);
    p_.h_in = p_.own.pinned<uint8_t>((size_t)V * H * W * 3);
    p_.d_bgr = p_.own.device<uint8_t>((size_t)V * H * W * 3 + 16);  // (+16: k_fn_front fetches a pixel as the two aligned words around it)
    unsigned *d_state = p_.own.device<unsigned>(16);       // four 4-word slots (the fused-scan form keeps one per level)
    unsigned *d_hist = p_.own.device<unsigned>(3 * 2048);  // one histogram per level (the k_scan form uses the first only)
    DR_HIP(hipMemset(d_hist, 0, 3 * 2048 * 4));
    DR_HIP(hipMemset(d_state, 0, 16 * 4));

    FeatureNetOps fn = build_featurenet("", V, H, W);
    p_.ops = std::move(fn.ops);
    p_.fork_lo = fn.fork_lo; p_.fork_hi = fn.fork_hi; p_.feat2_op = fn.feat2_op;
    if (fcache_cap_ > 0) build_fn1(H, W);

    Sink k{p_.ops, ""};
    for (int s = 1; s <= 3; ++s) {
      const int sc = 1 << (3 - s), h = H / sc, w = W / sc, D = blob_.depth_num[s - 1], C = 32 >> (s - 1);
      if (!(D == 4 || D % 8 == 0)) fail(DR_ERR_UNSUPPORTED, "depth_num[%d]=%d must be 4 or a multiple of 8", s - 1, D);
      const std::string S = std::to_string(s), cr = "cost_regularization_net.stage" + S + ".", pre = "s" + S + ".";
      DevTensor &vol = alloc(k, "volume" + S, D, h, w, C);
      if (C == 32 && sw_.vol_split && !conv_bf3_policy()) vol.split = 16;  // (the bf16 x 3 mode stages through its own kernel: one tensor)
      {
        Op o; o.kind = Op::COSTVOL; o.stage = s; o.name = pre + "costvol";
        o.bytes = 4.0 * ((double)V * h * w * C + vol.n());
        o.flops = (double)(V - 1) * D * h * w * (3.0 * C + 2.0 * C + 8.0 * C);  // diff^2, gate dot, weighted accumulate, 4-tap lerp
        k.ops.push_back(o);
      }
      const bool four = D == 4;
      DevTensor &c0 = cbr3(k, pre + "conv0", cr + "conv0", vol, 1, 1, CONV_XPAIR);
      DevTensor &k1 = cbr3(k, pre + "conv1", cr + "conv1", c0, 2, 2, CONV_NORMAL);
      DevTensor &k2 = cbr3(k, pre + "conv2", cr + "conv2", k1, 1, 1, CONV_NORMAL);
      DevTensor &k3 = cbr3(k, pre + "conv3", cr + "conv3", k2, 2, 2, CONV_NORMAL);
      DevTensor &k4 = cbr3(k, pre + "conv4", cr + "conv4", k3, 1, 1, CONV_NORMAL);
      DevTensor &k5 = cbr3(k, pre + "conv5", cr + "conv5", k4, four ? 1 : 2, 2, CONV_NORMAL);
      DevTensor &k6 = cbr3(k, pre + "conv6", cr + "conv6", k5, 1, 1, CONV_NORMAL);
      DevTensor &x7 = dbr3(k, pre + "conv7", cr + "conv7", k6, four ? 1 : 2, k4);
      DevTensor &x9 = dbr3(k, pre + "conv9", cr + "conv9", x7, 2, k2);
#ifdef DR_PARITY_HOOKS
      const HostTensor &w11 = blob_.at(cr + "conv11.conv.weight");
      const HostTensor &wpr = blob_.at(cr + "prob.weight");
      const bool tail = sw_.tail_fused && !sw_.prob_on_conv && !conv_bf3_policy() && w11.dims.size() == 5 && w11.dims[0] == 16 && w11.dims[1] == 8 && w11.dims[2] == 3 &&
                        w11.dims[3] == 3 && w11.dims[4] == 3 && x9.C == 16 && c0.C == 8 && x9.D * 2 == D && x9.H * 2 == h && x9.W * 2 == w && wpr.dims[0] == 1 && wpr.dims[1] == 8;
      if (tail) {
        // conv11 (ConvTranspose3d 16 -> 8 + BN + ReLU, + conv0) and prob (8 -> 1) in one z-marching launch: the 8-channel full-resolution tensor
        // between them (78.6 MB at stages 2 and 3) is never written or read (tail_kernels.h)
        std::vector<float> sc, bi;
        fold_bn(blob_, cr + "conv11.bn", 8, sc, bi);
        sc.insert(sc.end(), bi.begin(), bi.end());
        DevTensor &lg = alloc(k, "logits" + S, D, h, w, 1);
        Op o; o.kind = Op::TAIL; o.stage = s; o.name = pre + "tail";
        TailArgs &t = o.tail;
        t.x = x9.d; t.skip = c0.d; t.out = lg.d; t.D = D; t.h = h; t.w = w;
        t.wd = p_.arena.upload(tail_pack_deconv(w11.data.data()));
        t.sb = p_.arena.upload(sc);
        t.wp = p_.arena.upload(tail_pack_prob(wpr.data.data()));
        const bool mf = sw_.tail_fused == 1;
        t.wmf = mf ? p_.arena.upload(tail_pack_deconv_mfma(w11.data.data())) : nullptr;
        tail_set_tile(t, sw_.tail_qy, sw_.tail_zchunk, mf);
        const double N = (double)D * h * w;
        o.flops = 2.0 * 3.375 * 16 * 8 * N + 2.0 * 216 * N;  // the algorithmic MACs of both layers (halo recomputation not counted)
        o.bytes = 4.0 * (x9.n() + c0.n() + lg.n());
        k.ops.push_back(o);
      } else
#endif
      {
      DevTensor &x11 = dbr3(k, pre + "conv11", cr + "conv11", x9, 2, c0);
      if (sw_.prob_on_conv && w % 8 == 0) {
        // A/B hook: the Cout = 1 head as 8 x-shifts per column on the MFMA kernel (CONV_X8, 50 % of the rows carry work);
        // measured against k_prob in profiles/r02_experiments.txt
        add_conv(k, pre + "prob", cr + "prob", "", false, false, x11, "logits" + S, 3, 3, 3, 1, 1, 1, false, CONV_X8, nullptr, 0);
      } else {
        DevTensor &lg = alloc(k, "logits" + S, D, h, w, 1);
        Op o; o.kind = Op::PROB; o.stage = s; o.name = pre + "prob";
        p_.pr[s - 1] = {x11.d, p_.arena.upload(prob_taps(blob_.at(cr + "prob.weight").data)), lg.d, D, h, w};
        o.flops = 2.0 * 216 * D * h * w; o.bytes = 4.0 * (x11.n() + lg.n());
        k.ops.push_back(o);
      }
      }
      alloc(k, "depth" + S, 1, h, w, 1);
      alloc(k, "conf" + S, 1, h, w, 1);
      { Op o; o.kind = Op::REGRESS; o.stage = s; o.name = pre + "regress"; o.bytes = 4.0 * ((double)D * h * w + 2.0 * h * w); o.flops = 8.0 * D * h * w; k.ops.push_back(o); }
    }
    p_.filt = {p_.T("depth3").d, p_.T("conf3").d, alloc(k, "edge", 1, H, W, 1).d, alloc(k, "depth", 1, H, W, 1).d, alloc(k, "confidence", 1, H, W, 1).d, d_state, d_hist,
               H * W, H, W, sw_.hist_blocks, sw_.filter_fused};
    { Op o; o.kind = Op::EDGE; o.name = "filter.edge"; o.bytes = 8.0 * H * W; k.ops.push_back(o); }
    for (int i = 0; i < 3; ++i) {
      Op o; o.kind = Op::HIST; o.level = i; o.name = "filter.hist" + std::to_string(i); o.bytes = 4.0 * H * W; k.ops.push_back(o);
      if (sw_.filter_fused) continue;  // (the scan of level i is the prologue of the next kernel: mvs_kernels.h k_hist_s / k_apply_s)
      Op q; q.kind = Op::SCAN; q.level = i; q.name = "filter.scan" + std::to_string(i); k.ops.push_back(q);
    }
    { Op o; o.kind = Op::APPLY; o.name = "filter.apply"; o.bytes = 20.0 * H * W; k.ops.push_back(o); }
    return std::move(plan_);
  }

  // where the layer helpers put what they make: the op list they append to, and the prefix of the tensor names they allocate under
  // ("c1." for the single-view FeatureNet of the feature cache: it builds into its own tensors)
  struct Sink {
    std::vector<Op> &ops;
    std::string prefix;
  };
  DevTensor &alloc(const Sink &k, const std::string &name, int D, int H, int W, int C, int pad = 0) {
    DevTensor t; t.D = D; t.H = H; t.W = W; t.C = C; t.pad = pad;
    const std::string key = k.prefix + name;
    t.d = p_.own.device<float>(t.n(), nullptr, key.c_str());
    if (pad) DR_HIP(hipMemset(t.d, 0, t.n() * 4));  // the border is written once, here; producers only touch the interior
    p_.tensors[key] = t;
    return p_.tensors[key];
  }

  // ---------------------------------------------------------------- layer construction
  // FeatureNet's skip connection (1x1 conv + bias + nearest-upsampled coarser level) on the streaming kernel k_skip_up;
  // DR_SKIP_ON_CONV=1 keeps it on the MFMA convolution kernel (A/B hook, and the path for other channel counts).
  DevTensor &add_skip(Sink &k, const std::string &opname, const std::string &wname, const DevTensor &in, const std::string &outname, const DevTensor &coarse) {
    const HostTensor &w = blob_.at(wname + ".weight");
    // (measured at 640x480x7: stage 3, Cin = 8: 0.141 -> 0.108 ms; stage 2, Cin = 16, a quarter of the pixels and twice the
    // weights per lane: 0.038 -> 0.073 ms, so that one stays where it was)
    if (!kParityHooks || sw_.skip_on_conv || w.dims[0] != 32 || w.dims[1] != in.C || in.C != 8 || coarse.C != 32 ||
        coarse.H * 2 != in.H || coarse.W * 2 != in.W)
      return add_conv(k, opname, wname, "", true, false, in, outname, 1, 1, 1, 1, 1, 1, false, CONV_NORMAL, &coarse, 2);
    DevTensor &out = alloc(k, outname, in.D, in.H, in.W, 32);
    Op o; o.kind = Op::SKIPUP; o.name = opname;
    const float *wd = p_.arena.upload(w.data);
    o.skip = {in.d, wd, p_.arena.upload(blob_.at(wname + ".bias").data), coarse.d, out.d, in.D, in.H, in.W, in.C};
    o.flops = 2.0 * in.C * 32 * in.n() / in.C; o.bytes = 4.0 * (in.n() + coarse.n() + out.n());
    k.ops.push_back(o);
    return out;
  }
  // Adds one convolution layer (possibly several launches) to the plan; returns the output tensor.
  DevTensor &add_conv(Sink &k, const std::string &opname, const std::string &wname, const std::string &bnname, bool conv_bias, bool relu,
                      const DevTensor &in, const std::string &outname, int k3d, int kh, int kw, int sd, int sh, int sw,
                      bool transposed, ConvMode mode, const DevTensor *add, int add_mode, const ConvFuse *fz = nullptr, int out_pad = 0) {
    const HostTensor &w = blob_.at(wname + ".weight");
    ConvLayer L;
    L.transposed = transposed;
    const int c_out = transposed ? w.dims[1] : w.dims[0], c_in_real = transposed ? w.dims[0] : w.dims[1];
    L.Cout = c_out; L.Cin = in.C;
    L.kd = k3d; L.kh = kh; L.kw = kw; L.sd = sd; L.sh = sh; L.sw = sw; L.relu = relu; L.out_pad = out_pad;
    std::vector<float> padded;
    if (c_in_real != in.C) {  // RGB -> RGB0: zero-pad the input-channel axis of the weights
      if (transposed || c_in_real > in.C) fail(DR_ERR_ARG, "%s: channel mismatch", opname.c_str());
      padded = pad_cin(w.data, c_out, c_in_real, in.C, k3d * kh * kw);
      L.weight = padded.data();
    } else L.weight = w.data.data();
    if (!bnname.empty()) fold_bn(blob_, bnname, c_out, L.scale, L.bias);
    else if (conv_bias) L.bias = blob_.at(wname + ".bias").data;
    ConvPlanOut P0;  // dims first
    {
      auto cz = axis_classes(k3d, sd, transposed, in.D), cy = axis_classes(kh, sh, transposed, in.H), cx = axis_classes(kw, sw, transposed, in.W);
      P0.outD = transposed ? in.D * sd : cz[0].npos; P0.outH = transposed ? in.H * sh : cy[0].npos; P0.outW = transposed ? in.W * sw : cx[0].npos;
    }
    DevTensor &out = alloc(k, outname, P0.outD, P0.outH, P0.outW, c_out, out_pad);
    emit_conv(k, opname, L, mode, in, out, add ? add->d : nullptr, add_mode, add ? (add_mode == 2 ? add->n() : out.n()) : 0, fz);
    return out;
  }
  // Plans layer L (in -> out, both existing tensors) and appends its launch(es) to the op list.
  void emit_conv(Sink &k, const std::string &opname, const ConvLayer &L, ConvMode mode, const DevTensor &in, DevTensor &out, const float *add_d, int add_mode,
                 size_t add_n, const ConvFuse *fz = nullptr) {
    const int k3d = L.kd, kh = L.kh, kw = L.kw;
    ConvFuse fzc{};
    if (fz) fzc = *fz;
    const bool fused = fz != nullptr;
    ConvPlanOut P = plan_conv(L, mode, in.d, in.D, in.H, in.W, in.C, out.interior(), add_d, add_mode, p_.arena, 0, fz, in.split);
    // the autotuner re-plans this layer with another candidate of the cost model's ranking (weights are kept alive; the arena is the plan's, as the op is)
    auto keep = std::make_shared<std::vector<float>>(L.weight, L.weight + (size_t)L.Cout * L.Cin * k3d * kh * kw);
    ConvLayer Lc = L;
    const float *in_d = in.d;
    float *out_d = out.interior();
    const int iD = in.D, iH = in.H, iW = in.W, iC = in.C, iS = in.split, ncand = P.ncand;
    DeviceArena *arena = &p_.arena;
    auto replan = [arena, keep, Lc, mode, in_d, iD, iH, iW, iC, iS, out_d, add_d, add_mode, fzc, fused](int rank) mutable {
      Lc.weight = keep->data();
      return plan_conv(Lc, mode, in_d, iD, iH, iW, iC, out_d, add_d, add_mode, *arena, rank, fused ? &fzc : nullptr, iS).launches.at(0);
    };
    int idx = 0;
    for (auto &cl : P.launches) {
      Op o; o.kind = Op::CONV; o.conv = cl; o.name = opname + (P.launches.size() > 1 ? "." + std::to_string(idx) : "");
      if (P.launches.size() == 1) {
        o.replan = replan; o.ncand = ncand;
        char sig[160];
        snprintf(sig, sizeof sig, "%d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d", L.Cin, L.Cout, k3d, kh, kw, L.sd, L.sh, L.sw, L.transposed ? 1 : (L.up2 ? 1 + L.up2 : 0),
                 (int)mode + (fused ? 8 : 0) + (iS ? 16 : 0), iD, iH, iW);
        o.sig = sig;
      }
      o.flops = cl.flops;
      if (idx == 0) o.bytes = 4.0 * ((fused ? in.n() / in.C * fzc.cin + in.n() / 4 : in.n()) + out.n() + add_n);
      if (fused) o.flops += 2.0 * fzc.cin * in.C * (in.n() / in.C);
      k.ops.push_back(o);
      ++idx;
    }
  }
  // the fused FeatureNet kernels need 55 KB / 133.5 KB of dynamic LDS per workgroup: plan them only where the device grants that much to one
  // workgroup (on a part with less the launch would be rejected in every forward while the multi-launch forms still exist)
  bool lds_fits(size_t bytes) const {
    int optin = 0;
    if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, device_) != hipSuccess || optin <= 0) {
      (void)hipGetLastError();
      if (hipDeviceGetAttribute(&optin, hipDeviceAttributeMaxSharedMemoryPerBlock, device_) != hipSuccess) { (void)hipGetLastError(); return false; }
    }
    return (size_t)optin >= bytes;
  }
  // FeatureNet's first block: u8 BGR -> RGB0 / 255, conv0.0 (3 -> 8), conv0.1 (8 -> 8), both 3x3 + BN + ReLU (module.py:461-470).  One launch
  // (k_fn_front, fn_front.h) when the weights have that shape; DR_FN_FRONT=0, the bf16x3 mode and any other shape keep the three launches.
  DevTensor &front_block(Sink &k, const std::string &fn, int V, int H, int W) {
    const HostTensor &wa = blob_.at(fn + "conv0.0.conv.weight"), &wb = blob_.at(fn + "conv0.1.conv.weight");
    const bool shape_ok = wa.dims.size() == 4 && wa.dims[0] == 8 && wa.dims[1] == 3 && wa.dims[2] == 3 && wa.dims[3] == 3 &&
                          wb.dims.size() == 4 && wb.dims[0] == 8 && wb.dims[1] == 8 && wb.dims[2] == 3 && wb.dims[3] == 3;
    const bool fits32 = (double)V * H * W * 32.0 < 2147483648.0 && ((uintptr_t)p_.d_bgr & 3) == 0;  // (the kernel addresses both tensors with 32-bit byte offsets from an aligned base)
    if (!sw_.fn_front || conv_bf3_policy() || !shape_ok || !fits32 || !lds_fits(kFrontLdsBytes)) {
      DevTensor &img = alloc(k, "image", V, H, W, 4);
      { Op o; o.kind = Op::PREPROCESS; o.name = "preprocess"; o.bytes = (double)V * H * W * (3 + 16); o.pre = {p_.d_bgr, reinterpret_cast<float4 *>(img.d), lut_, (size_t)V * H * W}; k.ops.push_back(o); }
      DevTensor &c3a = cbr2(k, "fn.conv0.0", fn + "conv0.0", img, 3, 1, CONV_XPAIR);
      return cbr2(k, "fn.conv0.1", fn + "conv0.1", c3a, 3, 1, CONV_XPAIR);
    }
    DevTensor &c3 = alloc(k, "fn.conv0.1", V, H, W, 8);
    Op o; o.kind = Op::FRONT; o.name = "fn.front";
    FrontArgs &a = o.front;
    a.bgr = p_.d_bgr; a.lut = lut_; a.out = c3.d;
    a.w1 = reinterpret_cast<const float4 *>(p_.arena.upload(front_pack(wa.data.data(), 3, 4)));
    a.w2 = reinterpret_cast<const float4 *>(p_.arena.upload(front_pack(wb.data.data(), 8, 8)));
    auto affine = [&](const std::string &bn) {  // 16 scales, 16 biases: XPAIR row r = 8 * (x of the pair) + channel
      std::vector<float> sc, bi, sb(32);
      fold_bn(blob_, bn, 8, sc, bi);
      for (int r = 0; r < 16; ++r) { sb[r] = sc[r & 7]; sb[16 + r] = bi[r & 7]; }
      return p_.arena.upload(sb);
    };
    a.sb1 = affine(fn + "conv0.0.bn"); a.sb2 = affine(fn + "conv0.1.bn");
    a.V = V; a.H = H; a.W = W;
    a.tilesY = cdiv(H, kFrontTY); a.tilesX = cdiv(W, kFrontTXP); a.ntiles = V * a.tilesY * a.tilesX;
    o.flops = 2.0 * V * H * W * 9.0 * (4 * 8 + 8 * 8);  // (as the planner counts the two layers: RGB0 has four channels)
    o.bytes = (double)V * H * W * (3 + 32);
    k.ops.push_back(o);
    return c3;
  }
  DevTensor &cbr2(Sink &k, const std::string &name, const std::string &p, const DevTensor &in, int ks, int s, ConvMode m) {
    return add_conv(k, name, p + ".conv", p + ".bn", false, true, in, name, 1, ks, ks, 1, s, s, false, m, nullptr, 0);
  }
  DevTensor &cbr3(Sink &k, const std::string &name, const std::string &p, const DevTensor &in, int sd, int shw, ConvMode m) {
    return add_conv(k, name, p + ".conv", p + ".bn", false, true, in, name, 3, 3, 3, sd, shw, shw, false, m, nullptr, 0);
  }
  DevTensor &dbr3(Sink &k, const std::string &name, const std::string &p, const DevTensor &in, int sd, const DevTensor &skip) {
    return add_conv(k, name, p + ".conv", p + ".bn", false, true, in, name, 3, 3, 3, sd, 2, 2, true, CONV_NORMAL, &skip, 1);
  }

  // FeatureNet for a batch of V views (module.py:461-531), its tensors named prefix + ...
  FeatureNetOps build_featurenet(const std::string &prefix, int V, int H, int W) {
    FeatureNetOps out;
    Sink k{out.ops, prefix};
    const std::string fn = "feature_net.";
    DevTensor &c3 = front_block(k, fn, V, H, W);
    DevTensor &c2a = cbr2(k, "fn.conv1.0", fn + "conv1.0", c3, 5, 2, CONV_NORMAL);
    DevTensor &c2b = cbr2(k, "fn.conv1.1", fn + "conv1.1", c2a, 3, 1, CONV_NORMAL);
    DevTensor &c2 = cbr2(k, "fn.conv1.2", fn + "conv1.2", c2b, 3, 1, CONV_NORMAL);
    DevTensor &c1a = cbr2(k, "fn.conv2.0", fn + "conv2.0", c2, 5, 2, CONV_NORMAL);
    DevTensor &c1b = cbr2(k, "fn.conv2.1", fn + "conv2.1", c1a, 3, 1, CONV_NORMAL);
    DevTensor &c1 = cbr2(k, "fn.conv2.2", fn + "conv2.2", c1b, 3, 1, CONV_NORMAL);
    // feature maps handed to the cost volume carry a one-pixel zero border (k_costvol2); DR_COSTVOL_V1=1: the unpadded layout + k_costvol
    const int fpad = sw_.costvol_v1 ? 0 : 1;
    add_conv(k, "fn.out1", fn + "out.stage1", "", false, false, c1, "feat1", 1, 1, 1, 1, 1, 1, false, CONV_NORMAL, nullptr, 0, nullptr, fpad);
    out.fork_lo = k.ops.size();
    DevTensor &i2 = add_skip(k, "fn.skip2", fn + "skip.stage2", c2, "inter2", c1);
    add_conv(k, "fn.out2", fn + "out.stage2", "", false, false, i2, "feat2", 1, 3, 3, 1, 1, 1, false, CONV_NORMAL, nullptr, 0, nullptr, fpad);
    out.feat2_op = k.ops.size() - 1;
    // stage 3: skip.stage3 (1x1, 8 -> 32, + upsampled inter2) is computed inside out.stage3's staging step -- the
    // 32-channel full-resolution tensor between them (275 MB at 640x480x7) is never written or read.  DR_NO_SKIP_FUSION=1: the two-kernel path.
    const HostTensor &w3 = blob_.at(fn + "skip.stage3.weight");
    const HostTensor &wo3 = blob_.at(fn + "out.stage3.weight");
    // out.stage3 is linear in inter3 = up(inter2) + skip.stage3(c3) (no BatchNorm, no ReLU, no bias: module.py:480-485,524-529), so it
    // is evaluated as   conv3x3(c3; Wout . Wskip)  +  conv3x3(up(inter2); Wout)  +  (Wout . bskip, corrected at the image border):
    // an 8 -> 8 XPAIR layer at full resolution (composed weights), two 2 x 3-tap phase layers over inter2 at HALF resolution that
    // add their rows in place (ConvLayer::up2: the upsampled tensor never exists), and a border kernel.  11.0 GFLOP become 6.9, the
    // 275 MB inter3 and the skip staging disappear, and all three convolutions run on the persistent kernels (0.22 -> 0.13 ms).
    // feat3 then differs from the literal order by fp32 reassociation (2e-6 of its range).  DR_OUT3_FOLDED=0: the fused-skip form.
    if (sw_.out3_folded && !sw_.no_skip_fusion && !sw_.skip_on_conv && w3.dims[0] == 32 && w3.dims[1] == 8 && c3.C == 8 &&
        i2.C == 32 && wo3.dims[0] == 8 && wo3.dims[1] == 32 && i2.H * 2 == c3.H && i2.W * 2 == c3.W) {
      const Out3Fold fold = compose_out3(wo3.data, w3.data, blob_.at(fn + "skip.stage3.bias").data);
      const std::vector<float> &wa = fold.wa, &T = fold.T, &bint = fold.bint;
      DevTensor &f3 = alloc(k, "feat3", c3.D, c3.H, c3.W, 8, fpad);
      if (sw_.fn_head3 && !conv_bf3_policy() && (double)f3.n() * 4.0 < 2147483648.0 && (double)i2.n() * 4.0 < 2147483648.0 && lds_fits(kH3LdsBytes)) {  // one launch: the three terms meet in one accumulator (fn_head3.h)
        Op o; o.kind = Op::HEAD3; o.name = "fn.head3";
        Head3Args &a = o.head3;
        a.c0 = c3.d; a.i2 = i2.d;
        a.wa = reinterpret_cast<const float4 *>(p_.arena.upload(h3_pack_a(wa.data())));
        a.wb = reinterpret_cast<const float4 *>(p_.arena.upload(h3_pack_b(wo3.data.data())));
        std::vector<float> b16(16);
        for (int r = 0; r < 16; ++r) b16[r] = bint[r & 7];
        a.bias16 = p_.arena.upload(b16); a.T = p_.arena.upload(T);
        a.out = f3.interior(); a.V = c3.D; a.H = c3.H; a.W = c3.W;
        a.out_row = (f3.W + 2 * f3.pad) * 8; a.out_plane = (f3.H + 2 * f3.pad) * a.out_row;
        a.tilesY = cdiv(c3.H, kH3TY); a.tilesX = cdiv(c3.W, kH3TXP); a.ntiles = c3.D * a.tilesY * a.tilesX;
        o.flops = 2.0 * c3.D * c3.H * c3.W * (9.0 * 8 * 8 + 4.0 * 32 * 8);  // (as the four launches count them: 9 taps of the composed layer, 2 x 2 half-resolution pixels per output pixel)
        o.bytes = 4.0 * (c3.n() + i2.n() + (double)c3.D * c3.H * c3.W * 8);
        k.ops.push_back(o);
      } else {
      ConvLayer LA; LA.Cin = 8; LA.Cout = 8; LA.kd = 1; LA.kh = 3; LA.kw = 3; LA.weight = wa.data(); LA.bias = bint; LA.out_pad = fpad;
      emit_conv(k, "fn.out3a", LA, CONV_XPAIR, c3, f3, nullptr, 0, 0);
      for (int py = 0; py < 2; ++py) {
        ConvLayer LB; LB.Cin = 32; LB.Cout = 8; LB.kd = 1; LB.kh = 3; LB.kw = 3; LB.weight = wo3.data.data(); LB.up2 = 1 + py; LB.out_pad = fpad;
        emit_conv(k, py ? "fn.out3c" : "fn.out3b", LB, CONV_NORMAL, i2, f3, f3.interior(), 1, f3.n() / 2);
      }
      Op o; o.kind = Op::BORDERFIX; o.name = "fn.out3d";
      o.border = {f3.interior(), p_.arena.upload(T), c3.D, c3.H, c3.W, fpad};
      o.bytes = 64.0 * c3.D * (c3.H + c3.W);
      k.ops.push_back(o);
      }
    } else
    if (!sw_.no_skip_fusion && !sw_.skip_on_conv && kParityHooks && w3.dims[0] == 32 && w3.dims[1] == 8 && c3.C == 8 && i2.C == 32 &&
        i2.H * 2 == c3.H && i2.W * 2 == c3.W) {  // (parity build only: the fused-skip kernel instances are not in the product library)
      ConvFuse fz{c3.d, p_.arena.upload(w3.data), p_.arena.upload(blob_.at(fn + "skip.stage3.bias").data), i2.d, 8};
      DevTensor virt; virt.D = c3.D; virt.H = c3.H; virt.W = c3.W; virt.C = 32; virt.d = nullptr;  // inter3 exists in LDS only
      add_conv(k, "fn.out3", fn + "out.stage3", "", false, false, virt, "feat3", 1, 3, 3, 1, 1, 1, false, CONV_XPAIR, nullptr, 0, &fz, fpad);
    } else {
      DevTensor &i3 = add_skip(k, "fn.skip3", fn + "skip.stage3", c3, "inter3", i2);
      add_conv(k, "fn.out3", fn + "out.stage3", "", false, false, i3, "feat3", 1, 3, 3, 1, 1, 1, false, CONV_XPAIR, nullptr, 0, nullptr, fpad);
    }
    out.fork_hi = k.ops.size();
    return out;
  }

  // The single-view plan of the key-frame feature cache (mvs_cache.h has the whole story, in its opening comment): FeatureNet once more, for one view and into
  // tensors of its own ("c1."), every launch the batch plan's kernel instance for that layer; the entries; which launches store feat1..3, and where.
  void build_fn1(int H, int W) {
    if (p_.ops.empty() || p_.ops[0].kind != Op::FRONT || sw_.costvol_v1 || shard_nsrc_) return;  // (the single-view plan patches k_fn_front's image pointer per call)
    const std::string c1 = "c1.";
    p_.ops1 = build_featurenet(c1, 1, H, W).ops;
    if (!p_.match_fn1()) { p_.ops1.clear(); return; }
    // the entries: three bordered feature maps + the image, per cached key frame
    const size_t img_bytes = (size_t)H * W * 3;
    p_.fcache.resize(fcache_cap_);
    for (FcBuffers &e : p_.fcache) {
      for (int s = 0; s < 3; ++s) {
        const DevTensor &t = p_.T(c1 + "feat" + std::to_string(s + 1));
        e.feat[s] = p_.own.device<float>(t.n());
        DR_HIP(hipMemset(e.feat[s], 0, t.n() * 4));  // (the zero border is written once, here: the producers store interior pixels only)
      }
      e.bgr = p_.own.device<uint8_t>(img_bytes + 16);
    }
    // the single-view plan writes its three outputs straight into the entry of the image it runs on: which launches store into feat1..3, and where
    for (size_t i = 0; i < p_.ops1.size(); ++i) {
      Op &o = p_.ops1[i];
      float *out = o.kind == Op::CONV ? o.conv.args.out : (o.kind == Op::HEAD3 ? o.head3.out : nullptr);
      for (int s = 0; s < 3 && out; ++s) {
        const DevTensor &t = p_.T(c1 + "feat" + std::to_string(s + 1));
        if (out >= t.d && out < t.d + t.n()) p_.fn1_out.push_back({i, s, (size_t)(out - t.d)});
      }
    }
    if (p_.fn1_out.size() != 3) { p_.ops1.clear(); p_.fcache.clear(); }
  }

};

// What the engine's parts (mvs_stage.h, mvs_cache.h) read of the engine: references to members of its own, which outlive them.
struct MvsCore {
  const MvsSwitches &sw;
  const int &device;
  HipOwner &own;
  const hipStream_t &stream;
  const std::unique_ptr<MvsPlan> &plan;  // of the window shape H x W x V; null while the engine is not configured
  WindowArgs &win;                       // of the staged window
  const int &H, &W, &V;
};

}  // namespace dr
