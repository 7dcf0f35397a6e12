/* dr_mi355x.h -- C ABI of libdr_mi355x.so: the MI355X-native drop-in for TANDEM's libdr
 * operator API (DrMvsnet + DrFusion).  Plain pointers and sizes only; no torch / HIP types.
 *
 * Every entry point below replaces one member of the reference's C++ interface
 *   tandem/libdr/dr_mvsnet/src/dr_mvsnet/dr_mvsnet.h   (class DrMvsnet, DrMvsnetOutput)
 *   tandem/libdr/dr_fusion/src/dr_fusion/dr_fusion.h   (class DrFusion, DrFusionOptions, DrMesh)
 * The header-compatible C++ shim classes that forward to this ABI live in
 * tandem_amd/libdr/{dr_mvsnet.h,dr_fusion.h}; INTEGRATION.md shows how TANDEM links them.
 *
 * Error convention: the reference prints and exit()s on protocol violations and has no return
 * codes (dr_mvsnet.cpp:100-102,156-157; tsdf_volume.cu:520-524).  The C ABI returns an int
 * status instead (0 = ok) and keeps the message in dr_last_error(); the C++ shim reproduces the
 * reference's exit(EXIT_FAILURE) behaviour on non-zero status.
 */
#ifndef DR_MI355X_H
#define DR_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  DR_OK = 0,
  DR_ERR_ARG = 1,       /* bad argument (null pointer, aliasing views, unsupported size) */
  DR_ERR_PROTOCOL = 2,  /* call-order violation (reference: exit(EXIT_FAILURE)) */
  DR_ERR_DEVICE = 3,    /* HIP error / no GPU */
  DR_ERR_IO = 4,        /* a file is missing, malformed or cannot be written (weight blob, mesh, map file) */
  DR_ERR_CAPACITY = 5,  /* hash table / block pool exhausted (reference: KERNEL_ABORT trap, heap.cu:16) */
  DR_ERR_UNSUPPORTED = 6
};

/* Thread-local message of the last failing call in this thread ("" if none). */
const char *dr_last_error(void);
/* Library version string, e.g. "dr_mi355x 0.1 gfx950". */
const char *dr_version(void);

/* ------------------------------------------------------------------ DrMvsnet */
typedef struct drm_s drm_t;

/* DrMvsnet::DrMvsnet(char const* filename)                      dr_mvsnet.h:38, dr_mvsnet.cpp:20-26
 * `weights_path` names a TDMW blob (tandem_amd/weights.py) instead of a TorchScript archive. */
int drm_create(const char *weights_path, int device, drm_t **out);
/* DrMvsnet::~DrMvsnet(): waits for pending work, joins the worker  dr_mvsnet.cpp:28-38 */
void drm_destroy(drm_t *h);
/* DrMvsnet::CallAsync(...)                                      dr_mvsnet.h:43-53, dr_mvsnet.cpp:125-283
 * bgrs[v] -> H*W*3 u8 interleaved BGR; K9 row-major full-res intrinsics; c2ws[v] -> 16 floats
 * row-major camera-to-world.  Inputs are copied before return.  Blocks while the previous call
 * is still being processed ("Blocking for last input. Non-blocking for this input").
 * Returns DR_ERR_ARG if two bgr / c2w pointers alias (reference: exit, :153-160). */
int drm_call_async(drm_t *h, int height, int width, int view_num, int ref_index,
                   const uint8_t *const *bgrs, const float *K9, const float *const *c2ws,
                   float depth_min, float depth_max, float discard_percentage);
/* DrMvsnet::Ready()  non-blocking, 1 = no unprocessed input      dr_mvsnet.h:62, dr_mvsnet.cpp:54 */
int drm_ready(drm_t *h);
/* DrMvsnet::Wait()   blocking                                    dr_mvsnet.h:59, dr_mvsnet.cpp:109-119 */
int drm_wait(drm_t *h);
/* DrMvsnet::GetResult()  blocking; fills four caller-owned H*W float arrays (the members of
 * DrMvsnetOutput, dr_mvsnet.h:12-34).  A second call without a new drm_call_async returns
 * DR_ERR_PROTOCOL (reference: exit, dr_mvsnet.cpp:100-103). */
int drm_get_result(drm_t *h, float *depth, float *confidence, float *depth_dense, float *confidence_dense);
/* The operator boundary without its two host copies (no reference counterpart; DrMvsnet::GetResultView / AllocImage in the shim):
 * drm_get_result_view = drm_get_result returning POINTERS into the page-locked block the device wrote the four maps to (no 4.9 MB copy).
 * Two blocks alternate: the maps stay valid while the next drm_call_async is processed and are overwritten by the one after it; they
 * die with the engine and with a change of resolution.  Same protocol errors as drm_get_result.
 * drm_host_alloc / drm_host_free = page-locked host memory.  When EVERY image of a drm_call_async lives in page-locked memory (from
 * here, hipHostMalloc or hipHostRegister) the upload reads it in place instead of gathering the window into the engine's own staging
 * block first; the call still returns only after the copies have completed, so the caller may reuse the images at once. */
int drm_get_result_view(drm_t *h, const float **depth, const float **confidence, const float **depth_dense, const float **confidence_dense);
void *drm_host_alloc(size_t bytes);
void drm_host_free(void *p);

/* Extension (no reference counterpart): the KEY-FRAME FEATURE CACHE.  TANDEM's sliding window re-sends six of its seven images with every key frame
 * (ref: tandem/src/FullSystem/FullSystem.cpp:1162-1171 pushes frameHessians[i]->image_bgr for every active key frame), and FeatureNet
 * (ref: cva_mvsnet/models/module.py:496-531) is per image.  drm_set_feature_cache(h, capacity) makes the engine keep the three feature maps (and the
 * u8 image) of the last `capacity` images (0 = off, the default; capacity must exceed the window's view count): a window of which at most one image
 * is new runs FeatureNet on that one view.  A hit is found by a 128-bit key over a sample of the image and made exact on the device: every uploaded
 * image is compared byte for byte with the cached copy, and a difference drops the cache and repeats the window without it before a result leaves the
 * engine.  Results are bit-identical with the cache on and off.  Call it before the first window; changing it on a configured engine re-plans the
 * engine (upload the window again).  drm_feature_cache_stats: out[0] views answered by the cache, [1] views computed, [2] windows that took the batch
 * path, [3] key collisions caught by the device compare, [4] 1 if the single-view plan exists for the current window shape, [5] entries. */
int drm_set_feature_cache(drm_t *h, int capacity);
int drm_feature_cache_stats(drm_t *h, uint64_t out[6]);

/* --- device-resident / measurement / introspection hooks (no reference counterpart) --- */
/* Upload a window (same arguments as drm_call_async) and keep it resident in HBM. Synchronous. */
int drm_upload(drm_t *h, int height, int width, int view_num, int ref_index, const uint8_t *const *bgrs,
               const float *K9, const float *const *c2ws, float depth_min, float depth_max,
               float discard_percentage);
/* Enqueue `iters` complete forwards (pre-process .. edge filter) of the resident window on the
 * engine stream; returns after a stream synchronise.  ms_total (may be NULL) = hipEvent time. */
int drm_forward(drm_t *h, int iters, float *ms_total);
/* Autotune the convolution plan of the resident window: time the first max_candidates tile/pass configurations of each
 * layer's cost-model ranking on the device and keep the fastest.  before_ms / after_ms (may be NULL) = summed layer time.
 * Opt-in: a tuned engine's results differ from an untuned one's at the 1e-7 level (fp32 accumulation order). */
int drm_autotune(drm_t *h, int max_candidates, float *before_ms, float *after_ms);
/* --- view sharding (BASELINE configs[2]): one source view (or a few) per GPU, the host sum-reduces the
 * partial cost volumes over the ranks (RCCL).  No reference counterpart: the reference has no inference-time
 * collective.  Protocol per rank: drm_set_view_shard(total source views of the window) -> drm_upload(sub-window =
 * [reference view, this rank's source views], view_num may be 1) -> for p in 0..2 { drm_forward_phase(p);
 * all-reduce(sum) the tensor "volume<p+1>" in place } -> drm_forward_phase(3) -> drm_download.  With the shard set,
 * each rank's cost volume is sum_over_local_views((gate + 1) * (warp - ref)^2) / total, so the reduced volume is the
 * unsharded one up to fp32 summation order.  View-aggregation models only (module.py:1097-1108). */
int drm_set_view_shard(drm_t *h, int nsrc_total); /* 0 = off (default) */
/* Enqueue phase 0..3 of the resident window and wait for it: 0 = pre-process, FeatureNet, cost volume 1;
 * p = 1,2: regularise + regress stage p, cost volume p+1; 3 = regularise + regress stage 3, edge filter. */
int drm_forward_phase(drm_t *h, int phase);
/* The same collective INSIDE the engine, for hosts without a collective library of their own (TANDEM's C++ back-end):
 * rank 0 draws an id (drm_comm_unique_id) and hands the 128 bytes to every rank by any means; each rank calls
 * drm_comm_init on its engine (RCCL communicator on the engine's device, librccl bound with dlopen).  From then on a
 * sharded window (drm_set_view_shard > 0) needs no host step between phases: drm_call_async / drm_forward enqueue, on
 * the engine's stream, each cost-volume kernel followed by ncclReduce(sum) of that volume to rank 0; rank 0 alone
 * regularises and regresses the stage and ncclBroadcast()s its depth map (stage 3: depth and confidence) -- what the next
 * stage's hypotheses hang on -- back to every rank, so all ranks end with the same four output maps.  ((n-1)/n x 354 MB per
 * depth map over xGMI instead of an all-reduce's 2(n-1)/n; DR_SHARD_ALLREDUCE=1 selects the all-reduce
 * form, in which every rank regularises redundantly.)  FeatureNet's stage-2/3 heads overlap the first reduce on the side
 * stream.  Use at most as many ranks as the window has source views.  drm_forward_phase keeps the host-reduced protocol. */
int drm_comm_available(void);                /* DR_OK when RCCL (librccl.so.1, or $DR_RCCL_LIB) can be bound in this process */
int drm_comm_unique_id(uint8_t id[128]);
int drm_comm_init(drm_t *h, int rank, int world, const uint8_t id[128]);
int drm_comm_destroy(drm_t *h);
/* Ranks of the engine's communicator as RCCL reports them (ncclCommCount): 0 = no communicator, -1 = the bound library lacks the call. */
int drm_comm_count(drm_t *h, int *nranks);
/* Device pointer and element count of a named internal tensor ("volume1".."volume3", "feat1", "depth2", ...) AS IT LIES IN
 * MEMORY: "feat1".."feat3" carry a one-pixel zero border in H and W (the cost-volume kernels read them that way), so for
 * those the pointer is the padded base and *nfloats = V * (H + 2) * (W + 2) * C; "volume1" (32 channels) is stored as two consecutive
 * (D, H, W, 16) halves (channels 0-15 | 16-31).  drm_get_tensor returns the logical (D, H, W, C) block in every case. */
int drm_device_tensor(drm_t *h, const char *name, void **dptr, size_t *nfloats);
/* Copy the last forward's stage-3 outputs to host (same four arrays as drm_get_result). */
int drm_download(drm_t *h, float *depth, float *confidence, float *depth_dense, float *confidence_dense);
/* Unfiltered depth / confidence of stage 1..3 (h_s*w_s floats each). */
int drm_get_stage_output(drm_t *h, int stage, float *depth, float *confidence);
/* Named internal tensor of the last forward, copied to host in its device layout (channels-last).
 * n_max = capacity of out in floats; *n = element count; dims[4] = {D|V, H, W, C}. */
int drm_get_tensor(drm_t *h, const char *name, float *out, size_t n_max, size_t *n, int dims[4]);
/* Per-kernel timing of one forward (hipEvents around every launch). names: '\n'-separated. */
int drm_profile(drm_t *h, char *names, size_t names_cap, float *ms, int cap, int *count);
/* Algorithmic work of one forward of the resident window (SURVEY.md 8d "layer-boundary" model). */
int drm_work(drm_t *h, double *flops, double *bytes);

/* Kernel unit-test hook: run one convolution layer through the engine's packer + MFMA kernel.
 * in  : (D,H,W,Cin) channels-last, host.  weight: torch layout (Cout,Cin,kd,kh,kw) for conv,
 * (Cin,Cout,kd,kh,kw) for transposed.  scale/bias: per-Cout affine applied before ReLU (may be NULL).
 * add : optional residual, output-shaped (or (D,H/2,W/2,Cout) when add_up2).  out: (Do,Ho,Wo,Cout). */
int drm_debug_conv(int device, const float *in, int D, int H, int W, int Cin, const float *weight, int Cout,
                   int kd, int kh, int kw, int sd, int sh, int sw, int transposed, const float *scale,
                   const float *bias, int relu, const float *add, int add_up2, float *out, int out_dims[3]);

/* Kernel unit-test hook for the fused tail of CostRegNet (conv11 + prob in one launch, csrc/tail_kernels.h; cva_mvsnet/models/module.py:571-575,598-599):
 * x (D/2, h/2, w/2, 16) and skip (D, h, w, 8) channels-last, host; w_deconv (16, 8, 3, 3, 3) and w_prob (1, 8, 3, 3, 3) in torch layout; scale8 / bias8 =
 * the folded BatchNorm of conv11; qy / zchunk: tile and depth-chunk overrides (0: chosen by size); form: 1 = the transposed convolution on the matrix pipe
 * (k_tail_m), 0 = on the vector pipe (k_tail).  out: (D, h, w) logits. */
int drm_debug_tail(int device, const float *x, const float *skip, const float *w_deconv, const float *scale8, const float *bias8, const float *w_prob, int D,
                   int h, int w, int qy, int zchunk, int form, float *out);

/* Kernel unit-test hooks for the last two operators of the depth pipeline, run alone on data the caller chooses.  All arrays are host memory.  The kernel is
 * chosen from the environment switches by the engine's own rule and launched by the engine's own launcher (csrc/mvs_host.h choose_regress / choose_prob,
 * csrc/mvs_launch.h): DR_PROB_ZCHUNK and DR_HIST_BLOCKS in both libraries, DR_REGRESS_GENERIC, DR_PROB_REGRESS and DR_FILTER_FUSED in the parity library only (the
 * product ignores them, as its engine does; a choice that names a kernel the product does not contain answers DR_ERR_UNSUPPORTED).  Outputs no launch writes
 * keep the poison word of csrc/guard_host.h (a NaN).
 *
 * The hypothesis planes of both regression hooks (csrc/mvs_kernels.h PlaneArgs): prev == NULL: d_k = dmin + interval * k; else prev is the previous stage's depth
 * (hp, wp) = (h / 2, w / 2), cur its x2 bilinear upsampling, lo = max(cur - half_range, 1e-3), d_k = lo + full_range * (k / D).
 *
 * drm_debug_regress: logits (D, h, w) -> depth_out, conf_out (h, w) (module.py:1116-1133: softmax over D, its expectation over the planes, the sum of the four
 * probabilities around trunc(E[k])).  kernel_name_out (64 bytes, may be NULL): "k_regress_r<D>" or "k_regress". */
int drm_debug_regress(int device, const float *logits, int D, int h, int w, const float *prev, int hp, int wp, float dmin, float interval, float half_range,
                      float full_range, float *depth_out, float *conf_out, char kernel_name_out[64]);
/* drm_debug_prob_regress: x11 (D, h, w, 8) channels-last and w_prob (1, 8, 3, 3, 3) in torch layout -> logits_out (D, h, w), then the regression of those logits:
 * in the same launch where the engine would run it so (D = 8 in one z chunk: "k_prob2_regress<8>"), else as a second launch ("k_prob2<1>+k_regress_r<8>"). */
int drm_debug_prob_regress(int device, const float *x11, const float *w_prob, int D, int h, int w, const float *prev, int hp, int wp, float dmin, float interval,
                           float half_range, float full_range, float *logits_out, float *depth_out, float *conf_out, char kernel_name_out[64]);
/* drm_debug_edge_filter: the edge measure of depth (H, W) -> edge_out; the rank-th smallest edge value (0-based, rank < H W) by the three-level radix select ->
 * *thr_bits_out (its bit pattern); depth_out / conf_out = depth / conf with the pixels whose edge value is > that threshold set to 0.  The launch sequence is
 * the engine's (edge, three histogram levels, their scans as launches or as prologues, apply) on buffers of its own.  edge_in (may be NULL): copied over the
 * edge buffer behind the edge kernel and before the first level -- the select and the mask then run on these values (non-negative floats), and edge_out
 * returns them. */
int drm_debug_edge_filter(int device, const float *depth, const float *conf, int H, int W, const float *edge_in, unsigned rank, float *edge_out, float *depth_out,
                          float *conf_out, unsigned *thr_bits_out);

/* Test hooks of the parity library (libdr_mi355x_hooks.so); in the product library all three return DR_ERR_UNSUPPORTED.  With guards on, every
 * device allocation of the library (engine tensors, plan uploads, voxel pool, tracker arrays, dr_device_alloc, ...) lies between two guard bands of
 * guard_bytes each, and guards and payload start as a poison pattern in which every aligned 32-bit word is a quiet NaN (csrc/guard_host.h).  A guard
 * is compared with the pattern when its buffer is freed and by dr_guard_check; what differs is a violation: buffer label, payload bytes, side, first
 * and last byte offset relative to the payload edge (front: -1 is the byte before the payload; back: +0 the byte behind it), count.
 * dr_guard_set: guard_bytes a multiple of 4096, 0 = off; affects later allocations only.
 * dr_guard_check: scans every live guarded buffer and adds the violations found at frees since the last clear.  out = {live guarded buffers, buffers
 *   guarded since the last clear, violations, payload bytes of the live guarded buffers}; report (may be NULL): one line per violation, cut at cap.
 * dr_guard_clear: forgets the violations found at frees and restarts the count of guarded buffers. */
int dr_guard_set(size_t guard_bytes);
int dr_guard_check(uint64_t out[4], char *report, size_t cap);
int dr_guard_clear(void);

/* ------------------------------------------------------------------ DrFusion */
/* struct DrFusionOptions                                         dr_fusion.h:18-36 (same field order) */
typedef struct {
  float voxel_size;
  int num_buckets;
  int bucket_size;
  int num_blocks;
  int block_size;
  int max_sdf_weight;
  float truncation_distance;
  float max_sensor_depth;
  float min_sensor_depth;
  int num_render_streams;
  float fx, fy, cx, cy;
  int height, width;
} drf_options_t;

typedef struct drf_s drf_t;

/* DrFusion::DrFusion(DrFusionOptions const&)                     dr_fusion.h:46, dr_fusion.cpp:8-38 */
int drf_create(const drf_options_t *opt, int device, drf_t **out);
/* DrFusion::~DrFusion()                                          dr_fusion.cpp:41-46 */
void drf_destroy(drf_t *h);
/* DrFusion::IntegrateScanAsync(bgr, depth, pose)                 dr_fusion.h:50, tsdf_volume.cu:515-598
 * H*W*3 u8 BGR, H*W f32 metres (0 = invalid), 16-float row-major cam-to-world; inputs are copied
 * to pinned memory before return.  Wrong call order -> DR_ERR_PROTOCOL (reference: exit). */
int drf_integrate_scan_async(drf_t *h, const uint8_t *bgr, const float *depth, const float *pose16);
/* DrFusion::RenderAsync(std::vector<float const*>)               dr_fusion.h:52, tsdf_volume.cu:634-700
 * n must equal num_render_streams (may be 0). */
int drf_render_async(drf_t *h, const float *const *poses16, int n);
/* DrFusion::GetRenderResult(bgr, depth)                          dr_fusion.h:54, tsdf_volume.cu:702-737
 * Fills n library-owned pinned pointers, valid until the next drf_get_render_result. */
int drf_get_render_result(drf_t *h, uint8_t **bgr, float **depth, int n);
/* DrFusion::ExtractMeshAsync(lower, upper)                        dr_fusion.h:60, tsdf_volume.cu:759-779,
 * marching_cubes/mesh_extractor.cu:136-281.  Marching cubes over the lattice lower + g * voxel_size; legal where
 * IntegrateScanAsync is (after GetRenderResult); at most one extraction may be pending. */
int drf_extract_mesh_async(drf_t *h, const float lower[3], const float upper[3]);
/* DrFusion::GetMeshSync()                                         dr_fusion.h:61, tsdf_volume.cu:781-838
 * Waits for the pending extraction and copies it out: vert / cols hold num_max vertices (3 floats each);
 * *num = 3 * triangles; vert[9t + 3k + 0..2] = position of vertex k of triangle t, cols[...] = its colour as RGB in
 * [0, 1].  DR_ERR_CAPACITY if 3 * triangles > num_max (the mesh stays pending) or above 20 M triangles. */
int drf_get_mesh_sync(drf_t *h, size_t num_max, size_t *num, float *vert, float *cols);
/* Size of the pending mesh (waits for it, does not consume it) -- lets a binding allocate exactly; no reference
 * counterpart (the reference preallocates 2 x 720 MB, dr_fusion.cpp:36-37). */
int drf_mesh_num_triangles(drf_t *h, size_t *ntri);
/* DrFusion::SaveMeshToFile(filename, lower, upper)                dr_fusion.h:56, dr_fusion.cpp:74-93, mesh.cu:24-66
 * Synchronous extraction written as Wavefront OBJ: "v x y z r g b" per vertex, "f i i+1 i+2" per triangle. */
int drf_save_mesh(drf_t *h, const char *filename, const float lower[3], const float upper[3]);
/* Device pointers of render stream `stream`'s result (H*W*3 u8 BGR, H*W f32 depth), valid from drf_get_render_result
 * until the next drf_render_async; no reference counterpart.  Feeds drt_append_dense_reference(on_device = 1). */
int drf_get_render_device(drf_t *h, int stream, const uint8_t **d_bgr, const float **d_depth);
/* DrFusion::Synchronize()                                        dr_fusion.h:64 */
int drf_synchronize(drf_t *h);

/* --- introspection / measurement hooks (no reference counterpart) --- */
/* Counters: [0] allocated blocks, [1] voxels updated by the last scan (band + carve),
 * [2] voxels updated in total, [3] round-trip voxel mismatches (must stay 0). */
int drf_stats(drf_t *h, uint64_t out[4]);
/* Blocks the integration kernel has visited since creation (visible blocks of every scan; each is one 4 KB read whether or not a voxel of it was
 * updated): with out[2] of drf_stats the kernel's exact HBM bytes are 4096 * visited + 8 * updated. */
int drf_visited_blocks(drf_t *h, uint64_t *total);
/* Canonical dump for bit-exact comparison: coords[3*i..] block coordinates, voxels[4096*i..] the
 * 512 8-byte voxels {f32 sdf, u8 b,g,r, u8 weight} of block i in index order x*64+y*8+z. */
int drf_export_blocks(drf_t *h, int max_blocks, int32_t *coords, uint8_t *voxels, int *n);
/* The engine divides by voxel_size, fx and fy with a 3-instruction exact sequence (reciprocal + FMA correction) after
 * checking it against IEEE division for all 2^32 dividends at construction: *enabled = 1 if every check passed (else the
 * kernels use IEEE division), *mismatches = number of disagreeing dividends found. */
int drf_fast_div_status(drf_t *h, int *enabled, uint64_t *mismatches);
/* Test hook: out[i] = Combine(a[i], b[i], max_weight) evaluated by the integration kernel's own device function
 * (voxel.h:21-50), n 8-byte voxels {f32 sdf, u8 b,g,r, u8 weight} each -- lets a test sweep every colour/weight case. */
int drf_test_combine(drf_t *h, size_t n, const uint8_t *a, const uint8_t *b, int max_weight, uint8_t *out);
/* Integrate scans already resident in HBM (bench path): d_* are device pointers. */
int drf_integrate_device(drf_t *h, const void *d_bgr, const void *d_depth, const float *pose16);
/* Device-side scratch allocation helpers so a host without a HIP runtime binding can stage inputs. */
int dr_device_alloc(int device, size_t bytes, void **dptr);
int dr_device_free(void *dptr);
int dr_memcpy_h2d(void *dptr, const void *src, size_t bytes);
int dr_memcpy_d2h(void *dst, const void *dptr, size_t bytes);
int dr_memcpy_d2d(void *dst, const void *src, size_t bytes); /* returns after the copy has completed */
/* Time `iters` back-to-back integrations of `nscans` resident scans with hipEvents on the
 * integration stream.  ms / kernel_ms (integrate kernel only) may be NULL. */
int drf_bench_integrate(drf_t *h, const void *d_bgr, const void *d_depth, const float *poses16, int nscans,
                        float *ms, float *kernel_ms);

/* BASELINE configs[3] loop (dr_debug_example.cpp:78-162) over nframes frames resident in HBM (d_bgr: nframes*H*W*3 u8,
 * d_depth: nframes*H*W f32, poses16: nframes*16): allocate + integrate per frame and, if render != 0, one ray-cast per
 * render stream from the frame's pose with the D2H of its result.  ms[0] whole run (hipEvents), ms[1..4] sums of the
 * allocate / integrate / ray-cast / D2H intervals, ms[5] host wall clock. */
int drf_bench_sequence(drf_t *h, const void *d_bgr, const void *d_depth, const float *poses16, int nframes, int render, float ms[6]);
/* Test hook: host pointers (page-locked, library-owned) of the last (back = 0) / second-to-last (back = 1) render of `stream` written by
 * drf_bench_sequence.  In that loop the allocation of scan k + 1 runs beside the ray-cast of scan k (a device-resident sequence is the only
 * caller that reaches this overlap: through the operator API GetRenderResult(k) returns before IntegrateScanAsync(k + 1) is called). */
int drf_bench_render_host(drf_t *h, int stream, int back, const uint8_t **bgr, const float **depth);

/* --- streaming: a bounded device pool and a host store for the rest of the map (no reference counterpart; the reference's
 * HashTable::DeleteBlock / Heap::Append, hash_table.cu:117-139 and heap.cu:27, are never called by DrFusion).  DESIGN.md
 * "Streaming voxel blocks", INTEGRATION.md "Streaming".
 * Automatic mode (drf_set_streaming with radius > 0): each drf_integrate_scan_async / drf_integrate_device with camera centre p
 *   (1) folds the blocks evicted after the previous scan into the host store, (2) brings back every stored block whose
 *   centre ((8 b + 3.5) voxel_size per axis) lies within `radius` of p -- before the allocation pass --, (3) integrates
 *   unchanged, (4) evicts the resident blocks whose centre lies beyond radius + one block edge (8 voxel_size) of p.
 * Exactness contract: with radius >= drf_streaming_min_radius, the voxel state of the map (resident blocks plus host store)
 *   after every scan is bit-identical to an engine whose pool never runs out, and so are the update counts.
 * Renders read the RESIDENT blocks by default: a ray-cast then equals that engine's when its pose lies within
 *   radius - drf_streaming_min_radius of the last scan's camera centre (the scan pose itself always qualifies), and a farther
 *   one misses what is stored on the host.  After drf_set_render_scope(h, DRF_RENDER_MAP, ...) a ray-cast at ANY pose equals
 *   the unbounded engine's in depth and colour, without moving a block.
 * drf_export_blocks covers the RESIDENT blocks.  Mesh extraction covers them too by default; after
 *   drf_set_mesh_scope(h, DRF_MESH_MAP) it covers resident blocks and host store together, without moving a block.
 *   drf_bench_* return DR_ERR_UNSUPPORTED while streaming is on or the host store holds blocks, and integrating with
 *   streaming off while the host store holds blocks is DR_ERR_PROTOCOL. */
/* Smallest exact radius for these options: the farthest a block centre can lie from a scan's camera centre and still be
 * allocated, updated or ray-cast by it at the scan pose, plus one block diagonal; host-only, needs no device.
 * With rho = max |((u - cx)/fx, (v - cy)/fy, 1)| over the image corners and s = sqrt(3) * voxel_size:
 *   max(max_sensor_depth * rho + truncation_distance + 4.5 s, 12.5 s) + 8 s + voxel_size */
int drf_streaming_min_radius(const drf_options_t *o, float *radius);
/* radius = 0: off (the default).  A radius below drf_streaming_min_radius is DR_ERR_ARG; changing the mode while the host
 * store holds blocks is DR_ERR_PROTOCOL.  host_capacity_blocks bounds the host store (0 = unbounded): a region that does not
 * fit is DR_ERR_CAPACITY, and automatic eviction stops when the store is full (the pool then reports DR_ERR_CAPACITY). */
int drf_set_streaming(drf_t *h, float radius, size_t host_capacity_blocks);
/* Explicit moves of every block whose origin (8 b voxel_size per axis) lies in [lower, upper] (inclusive); legal where
 * drf_integrate_scan_async is, in either mode.  drf_stream_in_region that would not fit in the pool's free blocks returns
 * DR_ERR_CAPACITY and moves nothing; so does drf_stream_out_region that would not fit in the host store. */
int drf_stream_out_region(drf_t *h, const float lower[3], const float upper[3]);
int drf_stream_in_region(drf_t *h, const float lower[3], const float upper[3]);
/* out: [0] resident blocks, [1] blocks in the host store, [2] blocks streamed out, [3] blocks streamed in (totals),
 * [4] bytes moved (4096 per block either way), [5] device time of the last scan's stream-in and eviction launches in us
 * (0 when it had none). */
int drf_streaming_stats(drf_t *h, uint64_t out[6]);
/* The host store in the format of drf_export_blocks. */
int drf_export_host_blocks(drf_t *h, int max_blocks, int32_t *coords, uint8_t *voxels, int *n);
/* What drf_extract_mesh_async (with drf_mesh_num_triangles / drf_get_mesh_sync) and drf_save_mesh mesh.
 * DRF_MESH_RESIDENT (the default): the pool's blocks.  DRF_MESH_MAP: the pool and the host store together; the mesh equals,
 *   byte for byte and in the same triangle order (blocks by ascending packed key, then cells), the one an engine whose pool
 *   never ran out returns for the same scans and box.  It first folds pending evictions, then stages the host blocks it needs
 *   chunk by chunk through a bounded device scratch: the pool, its slot order, the host store and the streaming state stay
 *   unchanged, and it works with a full pool.  With an empty host store it is the resident pass.  DESIGN.md §7c.
 * A scope other than the two is DR_ERR_ARG; changing it while an extraction is pending is DR_ERR_PROTOCOL. */
enum { DRF_MESH_RESIDENT = 0, DRF_MESH_MAP = 1 };
int drf_set_mesh_scope(drf_t *h, int scope);
/* What drf_render_async ray-casts.  DRF_RENDER_RESIDENT (the default): the pool's blocks, exactly as without this call.
 * DRF_RENDER_MAP: the pool and the host store together -- every render equals, bit for bit in depth and colour, the one an
 *   engine whose pool never ran out returns for the same scans and pose.  Each drf_render_async selects the stored blocks its
 *   poses can read (the sphere of the ray-cast reach around each camera centre, cut by the view frustum; a pose that is not a
 *   finite rigid motion selects the whole store), stages their union through a device scratch of stage_capacity_blocks blocks
 *   (0 = min(num_blocks, 8192); 4104 bytes per block, twice) and ray-casts pool and staging together.  No block moves: pool,
 *   slot order, host store and streaming state stay as they were.  A union beyond the capacity makes drf_render_async return
 *   DR_ERR_CAPACITY with nothing changed (except that evictions the last scan left pending may already be folded into the host
 *   store, as every call that reads the store does) -- the call sequence still expects drf_render_async, which may be retried after a
 *   drf_set_render_scope with a larger capacity or in resident scope.  A render that cannot reach a block the last scan
 *   evicted does not wait for that scan; with no stored block in reach (an engine without streaming, the scan pose) the
 *   resident kernels run and nothing is copied.  DESIGN.md §7c "Rendering the whole map".
 * scope other than the two: DR_ERR_ARG; between drf_render_async and drf_get_render_result: DR_ERR_PROTOCOL */
enum { DRF_RENDER_RESIDENT = 0, DRF_RENDER_MAP = 1 };
int drf_set_render_scope(drf_t *h, int scope, size_t stage_capacity_blocks);
/* last drf_render_async: [0] stored blocks staged (union over its poses), [1] bytes uploaded,
   [2] poses that selected the whole store (not rigid), [3] 1 if it waited for the scan to fold evictions */
int drf_render_stats(drf_t *h, uint64_t out[4]);
/* Depth bands for map-scope renders whose union exceeds the staging (DESIGN.md §7c "Rendering beyond the staging").
 * max_passes 0 or 1: off (the default) -- every call behaves and launches as without this function.  2..64: such a
 *   drf_render_async stages and ray-casts up to max_passes consecutive slabs of camera depth one after the other, each within
 *   stage_capacity_blocks, the rays pausing at a slab's far side and resuming in the next pass.  The result equals the
 *   one-pass render bit for bit in depth and colour, and the same nothing moves.  A union that fits runs in one pass as before.
 *   DR_ERR_CAPACITY remains, with nothing changed, when the plan needs more than max_passes passes, when the thinnest possible
 *   band (about 2 x 12.5 sqrt(3) voxels + truncation_distance of depth) holds more blocks than the capacity, or when a pose that
 *   selects without the frustum cut (not a finite rigid motion; a reach beyond ~10^4 voxels) exceeds it on its own.
 * negative or above 64: DR_ERR_ARG; between drf_render_async and drf_get_render_result: DR_ERR_PROTOCOL */
int drf_set_render_bands(drf_t *h, int max_passes);
/* last drf_render_async: [0] passes (1 for an unbanded staged render, 0 when nothing was staged), [1] blocks staged by its
   largest pass, [2] blocks staged over all passes (a block staged by k passes counts k times; drf_render_stats [1] is
   4104 x this), [3] 1 if the render was banded */
int drf_render_band_stats(drf_t *h, uint64_t out[4]);
/* Last extraction: [0] blocks meshed (resident + stored), [1] host blocks uploaded (a block staged by k chunks counts k
 * times), [2] chunks (1 for a resident pass over a non-empty pool). */
int drf_mesh_stats(drf_t *h, uint64_t out[3]);

/* --- map files: the whole map -- resident blocks and host store -- saved to a file and loaded into a new engine (no reference
 * counterpart; DESIGN.md §7c "Saving and loading the map", INTEGRATION.md "Map files").
 * The file is a function of the map alone: every block of the map keyed by coordinate, blocks that were allocated and never
 * updated included, and nothing about the pool, slot order, streaming state, counters or options except voxel_size.  A bounded
 * streaming engine and an unbounded one write the same bytes after the same scans, and an engine that loads the file goes on
 * exactly where the saving engine stood: integration, update counts, ray-casts and meshes agree bit for bit.  Those
 * statements assume that the loading engine's other options (truncation distance, weights, depths, intrinsics) equal the
 * saving engine's: only voxel_size is recorded and checked.
 * Layout, little-endian, 72 + 4104 n bytes:
 *   offset 0          8 bytes magic "DRFMAP01"
 *          8          u32 header size = 64
 *          12         u32 block edge = 8
 *          16         u32 bytes per voxel = 8
 *          20         f32 voxel_size, stored as its bit pattern
 *          24         u64 n = number of blocks
 *          32         32 reserved bytes, all zero
 *          64         n x u64 packed block keys, STRICTLY ASCENDING: 21 bits per axis, each coordinate biased by 2^20, x in the
 *                     high bits -- ((x + 2^20) << 42) | ((y + 2^20) << 21) | (z + 2^20)
 *          64 + 8 n   n x 4096 bytes of voxels in the keys' order: per block 512 voxels {f32 sdf, u8 b, g, r, u8 weight} in
 *                     index order x*64 + y*8 + z, exactly what drf_export_blocks returns
 *          64 + 4104n u64 checksum over the key table and the voxel bytes, 8 bytes at a time: h = 0xcbf29ce484222325, then for
 *                     every little-endian u64 word w in file order h = (h ^ w) * 0x100000001b3 mod 2^64
 * chunk_blocks = blocks per transfer chunk (0 = min(num_blocks, 8192); never more than the map holds or 2^20): it bounds the
 * page-locked staging, two buffers of chunk_blocks * 4096 bytes.  Any file failure is DR_ERR_IO with the path in
 * dr_last_error(); a null argument is DR_ERR_ARG. */
/* Host-only, needs no device (like drf_streaming_min_radius): validates the WHOLE file -- size against n, magic, header size,
 * block edge, voxel bytes, reserved bytes, key order (and keys below 2^63), checksum -- and returns its voxel_size and n. */
int drf_map_info(const char *path, float *voxel_size, uint64_t *n_blocks);
/* Legal where drf_integrate_scan_async is (otherwise DR_ERR_PROTOCOL); a pending mesh extraction stays pending.  Like the
 * map-scope mesh pass it folds pending evictions first and is otherwise read-only: pool, slot order, host store, streaming
 * state, mesh-update baseline and all counters stay as they were.  Writes <path>.part and renames it on success, so a failed
 * save never leaves a truncated file under the requested name.  An empty map gives a valid 72-byte file. */
int drf_save_map(drf_t *h, const char *path, size_t chunk_blocks);
/* Legal where drf_integrate_scan_async is, on an engine whose map is EMPTY: a non-empty pool or host store, or a pending
 * eviction, is DR_ERR_PROTOCOL.  The whole file is validated first (DR_ERR_IO); a voxel_size whose bits differ from the
 * engine's is DR_ERR_ARG.  Streaming off: every block goes into the pool, slot i holding the block with the i-th key; more
 * blocks than num_blocks is DR_ERR_CAPACITY.  Streaming on: every block goes into the host store (more than
 * host_capacity_blocks: DR_ERR_CAPACITY) and the next scan brings in what lies within the radius, so the exactness contract
 * holds from the first scan; until then a resident-scope render sees nothing and a map-scope render (DRF_RENDER_MAP, and
 * likewise DRF_MESH_MAP) sees everything.  After a successful load, and until the next drf_integrate_scan_async,
 * drf_render_async is legal wherever drf_integrate_scan_async is, so a loaded map can be ray-cast from any pose before (or
 * without) a scan.  A failed load leaves the engine empty and usable.  A load makes the next mesh
 * update full, does not count as streamed in or out in drf_streaming_stats, and leaves the update counters of drf_stats at
 * zero ([0] reports the pool as always). */
int drf_load_map(drf_t *h, const char *path, size_t chunk_blocks);
/* Merges a map file into the map the engine holds, voxel by voxel (DESIGN.md §7c "Merging a map file"): two maps of the same
 * world -- same voxel_size, same world frame -- become one.  The rule:
 *   blocks  the merged map holds the union of the two block sets.  A file block whose key the map does not hold is placed
 *           verbatim, 4096 bytes unchanged, exactly as drf_load_map places it; one whose key the map holds is combined with the
 *           map's block voxel by voxel, index by index.
 *   voxels  a = the map's voxel, b = the file's, W = (unsigned char)max_sdf_weight, fp32 without contraction:
 *           1. b.weight == 0: a stays as it is, all 8 bytes.
 *           2. otherwise, a.weight == 0: a.sdf = b.sdf, a.colour = b.colour, a.weight = min(b.weight, W).
 *           3. otherwise, with wa = (float)a.weight, wb = (float)b.weight: each colour channel becomes
 *              (unsigned char)(((float)a.c * wa + (float)b.c * wb) / (wa + wb)), a.sdf = (a.sdf * wa + b.sdf * wb) / (wa + wb),
 *              a.weight = min((int)a.weight + (int)b.weight, (int)W).
 *           Case 3 is the reference's Voxel::Combine, except that the weight sum is formed in int (two unsigned chars would wrap
 *           above 255; integration adds 1 at a time and never gets there, a merge can).  Cases 1 and 2 keep 0/0 out of the map and
 *           make an absent block and an allocated block that was never updated behave the same.
 * Legal where drf_integrate_scan_async is (otherwise DR_ERR_PROTOCOL); a null argument is DR_ERR_ARG.  Folds pending evictions
 * first.  The whole file is validated before anything changes (DR_ERR_IO); a voxel_size whose bits differ from the engine's is
 * DR_ERR_ARG.  Capacity is decided before anything changes as well -- streaming off: resident blocks + added blocks must not
 * exceed num_blocks; streaming on: host-store blocks + added blocks must not exceed host_capacity_blocks when that is non-zero --
 * and DR_ERR_CAPACITY leaves pool, slot order, host store, counters and mesh baseline exactly as they were.
 * Streaming off: blocks whose key is resident are combined in their pool slots, blocks whose key is in the host store (after
 * drf_stream_out_region) are combined there, added blocks are appended behind the existing ones in ascending key order; the
 * order of the existing slots does not change.  Streaming on: resident keys are combined in the pool, stored keys in the host
 * store, new blocks go into the host store and the next scan brings in what lies within the radius, as after a load.
 * The merged map is a function of the two maps alone: whatever the pool size, the streaming state and chunk_blocks, engines
 * that held the same map and merge the same file save the same bytes, and an engine that merged goes on exactly like one that
 * loaded a file holding the merged map.  Merging into an empty engine is drf_load_map.
 * Afterwards the next mesh update is full; drf_stats [1] to [3] and the streaming counters do not move; a pending mesh
 * extraction stays pending and describes the map before the merge; until the next scan drf_render_async is legal wherever
 * drf_integrate_scan_async is, as after a load.
 * If the file changes between the validation and the second pass (a read fails or the checksum of what was read differs) the
 * call returns DR_ERR_IO and the map is a valid MIXTURE: every file block is either fully merged or untouched, drf_merge_stats
 * says how far it got, and the engine stays usable.  No rollback is attempted: it would need a copy of the map. */
int drf_merge_map(drf_t *h, const char *path, size_t chunk_blocks);
/* last drf_merge_map: [0] blocks in the file, [1] blocks added (key was not in the map), [2] blocks combined in the pool,
 * [3] blocks combined in the host store, [4] voxels of combined blocks taken verbatim (case 2), [5] voxels averaged (case 3) */
int drf_merge_stats(drf_t *h, uint64_t out[6]);
/* Moves a map file into another world frame (DESIGN.md §7c "Moving a map into another frame"): reads src_path, resamples its
 * surface on the engine's voxel lattice under the rigid motion T16 and writes the result to dst_path as a map file, which
 * drf_load_map and drf_merge_map then take like any other.  T16 is row-major and maps file-world to engine-world,
 * p_engine = R p_file + t, the convention of the poses.  The engine lends its device, its streams, its pinned buffers and its
 * voxel_size; its own map is neither read nor changed: pool, slot order, host store, streaming state, mesh baseline and every
 * counter stay as they were, a pending mesh extraction stays pending, and drf_save_map writes the same bytes before and after.
 * The rule, per destination lattice point g (a voxel with lattice coordinates g sits at g * voxel_size; block floor(g / 8),
 * index (gx & 7) * 64 + (gy & 7) * 8 + (gz & 7)).  Once, in double: Rd[i][j] = T16[4 i + j], tv[j] = T16[4 j + 3] / voxel_size.
 *   position  in double, without contraction: d = g - tv, u_k = (Rd[0][k] d_0 + Rd[1][k] d_1) + Rd[2][k] d_2 (= R^T d),
 *             b_k = floor(u_k), f_k = (float)(u_k - b_k).
 *   corners   c = 4 cx + 2 cy + cz with the fp32 weight w_c = (a_x(cx) * a_y(cy)) * a_z(cz), a_k(0) = 1.0f - f_k, a_k(1) = f_k.
 *             A corner is USED iff w_c != 0 and reads the source voxel at lattice point b + (cx, cy, cz); an absent block, or one
 *             outside the key range, counts as weight 0.
 *   result    if any used corner has weight 0: 8 zero bytes.  Otherwise sdf = the sum of w_c * sdf_c over the used corners in
 *             ascending c in fp32 (the first used term initialises the sum), each colour channel
 *             (unsigned char)min(sum of w_c * (float)channel_c + 0.5f, 255.0f) in the same order, weight = the smallest of the
 *             used corners' weights.  A partly weighted neighbourhood is refused, not renormalised.
 *   blocks    a destination block is written iff one of its 512 voxels has weight > 0, with all 4096 bytes as computed; keys
 *             strictly ascending.  The output is a function of the source file and T16 alone.
 * So a signed permutation matrix with a translation of whole voxels (voxel_size a power of two) moves every weighted voxel with
 * its 8 bytes unchanged, and the identity writes the source without its weight-0 voxels and its blocks that hold no other.
 * Scale is not handled: T16 must be rigid.
 * Legal where drf_integrate_scan_async is (otherwise DR_ERR_PROTOCOL).  DR_ERR_ARG: a null argument; src_path and dst_path the
 * same string; T16 with a non-finite entry, a last row that is not exactly 0 0 0 1, R R^T differing from I by 1e-3 or more in an
 * entry, or det R <= 0; a file whose voxel_size bits differ from the engine's; a motion that takes a candidate destination block
 * outside the 21-bit key range.  DR_ERR_IO: the source fails the whole-file validation (before anything else is done with it),
 * or any other file failure (the path is in dr_last_error()).  DR_ERR_CAPACITY: the source cannot be held on the device --
 * it is uploaded whole for the duration of the call, key table and voxels, 4104 n bytes, and freed before the call returns;
 * sources beyond the free device memory are out of scope and are refused with nothing written.  The output goes to <dst_path>.part and takes its name when it is complete: no failure leaves a partial file under
 * dst_path.  It streams through the engine's pinned buffers in chunks of chunk_blocks blocks (0: as drf_save_map).  An empty
 * source, or one that yields no weighted voxel, gives a valid file of 72 bytes. */
int drf_transform_map(drf_t *h, const char *src_path, const float T16[16], const char *dst_path, size_t chunk_blocks);
/* last drf_transform_map: [0] source blocks, [1] candidate destination blocks evaluated, [2] blocks written, [3] voxels written
 * with weight > 0, [4] destination voxels refused because only part of their neighbourhood was weighted, [5] device bytes held
 * for the source */
int drf_transform_stats(drf_t *h, uint64_t out[6]);
/* Registers one map file to another (DESIGN.md §7c "Registering two maps"): finds the rigid motion T, src-world to ref-world,
 * p_ref = R p_src + t -- the convention of drf_transform_map, so T16_out goes straight into drf_transform_map(h, src, T16_out, dst)
 * and the result into drf_merge_map of an engine that holds ref.  Both files are truncated signed distance fields of (partly) the
 * same surface; the call minimises, over the source voxels near the surface, the difference between the source's sdf and the
 * reference's sdf interpolated at the moved voxel (SDF-to-SDF, Gauss-Newton with Huber weights).  It REFINES: T_init must bring the
 * source surface inside the reference's truncation band (a few voxels, a few degrees across the map).  There is no damping, no
 * line search, no coarse-to-fine and no global search; a start outside the basin ends DRF_ALIGN_LOST or in a wrong minimum.
 * The engine lends its device, its streams, its pinned buffers and its voxel_size; its own map is neither read nor changed, exactly
 * as for drf_transform_map.  drf_align_system evaluates the system once at T16: the score of a pose hypothesis (sums[27] /
 * counts[1] is the mean robust squared residual in voxels^2; counts[1] / counts[0] the overlap).
 * The rule (one text, pose_host.h, compiled for the host and for the kernel; double and fp32 without contraction):
 *   motion    Rd[i][j] = T16[4 i + j], tv[j] = T16[4 j + 3] / voxel_size in double, as for drf_transform_map; during the iterations
 *             the pose is held as (Rd, tv) in double.
 *   centre    once, from the source's block coordinates, integers in double: c_src[k] = 4 (min_k + max_k + 1) (0 for an empty
 *             source); per evaluation c_k = ((Rd[k][0] c_src0 + Rd[k][1] c_src1) + Rd[k][2] c_src2) + tv_k.
 *   sample    a source voxel at lattice point g with weight >= min_weight and |sdf| <= band (fp32 compare).  In double:
 *             q_k = ((Rd[k][0] g0 + Rd[k][1] g1) + Rd[k][2] g2) + tv_k, b = floor(q), f = (float)(q - b); a q_k that is not
 *             within (-2^30, 2^30) makes the sample invalid.
 *   validity  the eight reference voxels at b + (cx, cy, cz) are read (the gradient needs all eight even where f_k == 0); the
 *             sample is VALID iff all eight have weight >= min_weight; an absent block, or one outside the key range, has weight
 *             0.  An invalid sample adds nothing to the sums and is counted in counts[2].
 *   field     fp32, s[cx][cy][cz] the eight sdf values, in this order:
 *               z: h[cx][cy] = s[cx][cy][1] - s[cx][cy][0];  e[cx][cy] = s[cx][cy][0] + fz * h[cx][cy]
 *               y: dy[cx] = e[cx][1] - e[cx][0];  d[cx] = e[cx][0] + fy * dy[cx];  hy[cx] = h[cx][0] + fy * (h[cx][1] - h[cx][0])
 *               x: phi = d[0] + fx * (d[1] - d[0]);  gx = d[1] - d[0];  gy = dy[0] + fx * (dy[1] - dy[0]);
 *                  gz = hy[0] + fx * (hy[1] - hy[0])
 *   residual  double: r = ((double)phi - (double)s_src) / (double)voxel_size, n_k = (double)g_k / (double)voxel_size with
 *             g = (gx, gy, gz) of the field, x = q - c, J = (x1 n2 - x2 n1, x2 n0 - x0 n2, x0 n1 - x1 n0, n0, n1, n2),
 *             a = |r|, w = a <= (double)huber ? 1.0 : (double)huber / a.
 *   sums      [0..20] += (w J_i) J_j for i <= j, row-major; [21..26] += (w J_i) r; [27] += (w r) r.
 *             counts = {samples, valid, invalid}.
 *   order     per source block, lane l of 64 adds its voxels v = 2 (l + 64 k) and v + 1 for k = 0..3 (voxel index
 *             x * 64 + y * 8 + z), in that order, to 28 doubles that start at +0.0; then x = x + x[lane ^ off] for off = 32, 16, 8,
 *             4, 2, 1; the block's 28 values are partial[i], i the block's index in the ascending key table.  Then per component
 *             lane l adds partial[l], partial[l + 64], ... in ascending order from +0.0, and the same butterfly gives the sum.
 *   step      H = the symmetric 6x6 of sums[0..20], b = sums[21..26].  Cholesky H = L L^T column by column: the pivot of column j
 *             is p = H[j][j] - L[j][0]^2 - ... - L[j][j-1]^2 (subtracted in that order); p <= 1e-12 * max_j H[j][j] (or a maximum
 *             that is not > 0) ends the call DRF_ALIGN_DEGENERATE.  L[j][j] = sqrt(p), L[i][j] = (H[i][j] - L[i][0] L[j][0] - ...
 *             - L[i][j-1] L[j][j-1]) / L[j][j]; y_i = (-b_i - L[i][0] y_0 - ... - L[i][i-1] y_{i-1}) / L[i][i];
 *             d_i = (y_i - L[i+1][i] d_{i+1} - ... - L[5][i] d_5) / L[i][i], i descending.  d = (omega, v).
 *             |omega| = sqrt((o0 o0 + o1 o1) + o2 o2) < eps_rot and |v| < eps_trans (same form): DRF_ALIGN_CONVERGED, the step is
 *             not applied.  Otherwise a = 1 / sqrt(1 + ((o0 o0 + o1 o1) + o2 o2) / 4), (qw, qx, qy, qz) = (a, (a o0) / 2,
 *             (a o1) / 2, (a o2) / 2), Rq the rotation matrix of that unit quaternion
 *               [1 - 2 (qy qy + qz qz), 2 (qx qy - qw qz), 2 (qx qz + qw qy); 2 (qx qy + qw qz), 1 - 2 (qx qx + qz qz),
 *                2 (qy qz - qw qx); 2 (qx qz - qw qy), 2 (qy qz + qw qx), 1 - 2 (qx qx + qy qy)],
 *             Rd' = Rq Rd with entries (Rq[i][0] Rd[0][j] + Rq[i][1] Rd[1][j]) + Rq[i][2] Rd[2][j], and with e = tv - c,
 *             tv'_k = (c_k + ((Rq[k][0] e0 + Rq[k][1] e1) + Rq[k][2] e2)) + v_k: a rotation about the centre.
 *   loop      evaluate; DRF_ALIGN_LOST if valid < min_valid * samples (in double) or valid < 6; else step; after max_iters
 *             evaluations DRF_ALIGN_MAX_ITERS.  Only + - * / sqrt and floor are used: no library function whose rounding
 *             could differ between hosts and the device.
 * What ends where: CONVERGED and DEGENERATE end on the pose of the last evaluation.  LOST ends on the last pose whose evaluation
 * was not lost (T_init if the first one was); sums, valid and cost then describe the lost evaluation.  MAX_ITERS applies the
 * step of its last evaluation: T is one step past the pose that sums, valid and cost describe.
 * Legality and refusals, in this order: a null argument (opt and res may be null) or an option that is negative or not finite,
 * DR_ERR_ARG; not where drf_integrate_scan_async is legal, DR_ERR_PROTOCOL; a T that drf_transform_map would refuse, DR_ERR_ARG;
 * a file that fails the whole-file validation, src first, DR_ERR_IO; a voxel_size whose bits differ from the engine's, src
 * first, DR_ERR_ARG; DR_ERR_CAPACITY when both maps do not fit on the device together: they are uploaded whole, once per call,
 * 4104 (n_src + n_ref) bytes plus 224 n_src + 32 for the partial sums and counters, and freed on every way out; a file that
 * changed between validation and upload, DR_ERR_IO.  src_path == ref_path is allowed (a self-score).
 * DR_OK means the call ran: a registration that ends DRF_ALIGN_DEGENERATE or DRF_ALIGN_LOST returns DR_OK with res->status set,
 * T16_out as described above and a message in dr_last_error(). */
typedef struct {
  int    max_iters;   /* 0 -> 30 */
  int    min_weight;  /* 0 -> 1; a voxel counts as observed iff weight >= min_weight */
  float  band;        /* metres; 0 -> 2 * voxel_size (fp32 product); source voxels with |sdf| <= band are samples */
  float  huber;       /* voxels; 0 -> 1.0 */
  double eps_rot;     /* rad; 0 -> 1e-7 */
  double eps_trans;   /* voxels; 0 -> 1e-5 */
  double min_valid;   /* share of the samples that must be valid; 0 -> 0.25 */
} drf_align_options_t;
enum { DRF_ALIGN_CONVERGED = 0, DRF_ALIGN_MAX_ITERS = 1, DRF_ALIGN_DEGENERATE = 2, DRF_ALIGN_LOST = 3 };
typedef struct {
  double   T[16];         /* row-major, src-world -> ref-world, metres: Rd, t_k = tv_k * (double)voxel_size, last row 0 0 0 1 */
  double   sums[28];      /* the last system evaluated */
  uint64_t samples, valid0, valid;   /* in band; valid at T_init; valid at the last evaluation */
  double   cost0, cost;   /* sums[27] / valid at T_init and at the last evaluation (0 where valid is 0) */
  int      iterations, status;  /* evaluations made; DRF_ALIGN_* */
} drf_align_result_t;
/* the system at T16: sums[28] and counts = {samples, valid, invalid} */
int drf_align_system(drf_t *h, const char *src_path, const char *ref_path, const float T16[16], const drf_align_options_t *opt,
                     double sums[28], uint64_t counts[3]);
/* the registration from T_init16; T16_out = res->T rounded to float (it passes drf_transform_map's test of a motion) */
int drf_align_map(drf_t *h, const char *src_path, const char *ref_path, const float T_init16[16], const drf_align_options_t *opt,
                  float T16_out[16], drf_align_result_t *res);
/* last drf_align_system / drf_align_map: [0] source blocks, [1] reference blocks, [2] samples, [3] valid samples at the last
 * evaluation, [4] system evaluations, [5] device bytes held during the call (all 0 after a call that was refused) */
int drf_align_stats(drf_t *h, uint64_t out[6]);
/* Locates a depth frame in the map the engine holds (DESIGN.md §7c "Locating a depth frame in the map"): the frame-to-model step.
 * One depth image (height x width floats, metres, as drf_integrate_scan_async takes it: a sensor frame, a DrMvsnet depth map, a
 * ray-cast) and a rough pose in, the refined pose in the map's frame out -- the pose16 that drf_integrate_scan_async needs to
 * continue a map brought in by drf_load_map, the start from which drf_transform_map and drf_merge_map bring a second session over,
 * and a per-frame drift check of a running session.  The call minimises, over the depth pixels, the map's sdf interpolated at the
 * pixel's point (depth-to-SDF, Gauss-Newton with Huber weights); it REFINES, as drf_align_map does: pose_init must bring the
 * points inside the truncation band.  No damping, no coarse-to-fine, no global search (from a pose that is only good to decimetres
 * and degrees call drf_track_frame, below, first: its basin is set by a projective association, not by the band, and it ends
 * inside this call's; with no pose at all but a place, drf_search_frame, further below, finds the start).  drf_locate_system evaluates the system
 * once at pose16: the score of a pose hypothesis (sums[27] / counts[1], counts[1] / counts[0]).
 * The map is read where it lives, through the dense grid and the far-block table: nothing is uploaded but the depth image (through
 * the engine's pinned input buffer; the _device forms take a device pointer as drf_integrate_device does -- a rendered depth from
 * drf_get_render_device, or the dense hand-off, never goes through the host).  The call runs on the integration stream, behind any
 * pending scan, and returns when it is done.  It neither changes the map nor allocates a block: drf_stats, the export and the next
 * render are bit-identical with and without it.
 * SCOPE (drf_set_locate_scope, below).  DRF_LOCATE_RESIDENT, the default: the resident map only.  With streaming on, blocks in the
 * host store read as absent (their samples are `unobserved`); drf_locate_stats()[5] tells how many there are.
 * DRF_LOCATE_MAP: the pool and the host store together -- sums, counts, result and pose are, bit for bit, those of an engine whose
 * pool holds the whole map, whatever the split between pool and store.  No block moves: the map, the store, the pool and the
 * streaming state are as the call found them (drf_stream_in_region, the other way to the stored blocks, moves them into the pool,
 * can fail with DR_ERR_CAPACITY and changes what the next scan evicts).
 *   selection  An evaluation at a pose reads, for each sample point p of the pixel pyramid (z <= max_sensor_depth), the eight
 *              lattice corners around it: blocks whose centre lies within 4.5 sqrt(3) voxel_size of p.  The call stages, through
 *              the staging of the map-scope render, the stored blocks that a DRF_RENDER_MAP render at that pose would stage: the
 *              same pyramid and sphere widened by (4.5 sqrt(3) + 8 sqrt(3) + 1) voxel_size, a superset with 8 sqrt(3) voxels
 *              to spare.  A block the pool holds is read from the pool; with an empty store or an empty selection nothing is
 *              staged and the call is the resident one.
 *   reuse      A staging made at pose A serves an evaluation at pose B while drift(A, B) = |tA - tB| + ||RA - RB||_F *
 *              max_sensor_depth * rho <= slack = 8 sqrt(3) voxel_size - 4e-3 * (max_sensor_depth * rho + the widening), rho the
 *              largest |((u - cx) / fx, (v - cy) / fy, 1)| over the image corners (fusion_host.h: locate_pose_drift,
 *              locate_stage_slack; DESIGN.md derives both).  A refinement that moves farther selects and stages again at B.
 *   capacity   stage_capacity_blocks of drf_set_locate_scope bounds one staging (0: min(num_blocks, 8192), the render's
 *              default); the staging buffer grows to the larger need of its two users.  A selection above it is refused with
 *              DR_ERR_CAPACITY before anything is evaluated (a later pose of a refinement whose selection exceeds it ends the
 *              call the same way); the message gives both counts.  Raise the capacity, or use drf_stream_in_region.  Depth bands
 *              (drf_set_render_bands) do not apply to this call.
 * The rule (one text, pose_host.h, compiled for the host and for the kernel; double and fp32 without contraction; only + - * /
 * sqrt and floor are used):
 *   pose      pose16 is the engine's own convention: row-major, camera-to-world, metres.  Rd[i][j] = pose16[4 i + j],
 *             tv[j] = pose16[4 j + 3] / voxel_size in double; during the iterations the pose is held as (Rd, tv) in double.
 *   grid      step >= 1 is a pixel stride: Wg = ceil(width / step), Hg = ceil(height / step); grid position n = j * Wg + i is
 *             pixel (u, v) = (step * i, step * j) with dep = depth[v * width + u].  It is a SAMPLE iff, in fp32 compares,
 *             dep > 0, dep >= min_sensor_depth and dep <= max_sensor_depth (a NaN is no sample): the pixels k_integrate uses.
 *   point     double, z = (double)dep, vs = (double)voxel_size: g0 = ((((double)u - (double)cx) / (double)fx) * z) / vs,
 *             g1 = ((((double)v - (double)cy) / (double)fy) * z) / vs, g2 = z / vs: the camera-frame point in lattice units,
 *             pixel centres at whole (u, v).  q_k = ((Rd[k][0] g0 + Rd[k][1] g1) + Rd[k][2] g2) + tv_k.  The lattice point g of
 *             the map sits at world g * voxel_size (what drf_integrate_scan_async and drf_transform_map use): no half-voxel
 *             offset, and not the ray-cast's dual-grid interpolation.
 *   field, validity, residual, sums: drf_align_map's from q on, with s_src = 0 -- b = floor(q), f = (float)(q - b), the eight
 *             voxels at b + (cx, cy, cz); a sample one of whose eight has weight < min_weight (an absent block: weight 0), or
 *             whose q is not within (-2^30, 2^30), is UNOBSERVED.  One addition: a sample whose eight corners are observed but
 *             whose fp32 |phi| < band is false is OUTSIDE (the flat region in front of a surface, where the gradient is zero).
 *             Neither adds to the sums.  r = (double)phi / vs.  counts = {samples, valid, unobserved, outside},
 *             samples = valid + unobserved + outside.
 *   centre    c_src = (0, 0, (double)centre_depth / vs); per evaluation c_k = ((Rd[k][0] c_src0 + Rd[k][1] c_src1) +
 *             Rd[k][2] c_src2) + tv_k.  centre_depth = 0 rotates about the camera centre; the scene's depth conditions the
 *             system better.
 *   order     group i covers grid positions 512 i .. 512 i + 511; lane l of 64 adds positions 512 i + l + 64 k, k = 0..7, in
 *             that order, to 28 doubles from +0.0 (positions >= Wg * Hg are no samples); then x = x + x[lane ^ off] for
 *             off = 32, 16, 8, 4, 2, 1 gives partial[i]; then drf_align_map's fold over the groups.
 *   step, loop, statuses: drf_align_map's, unchanged (DRF_ALIGN_*), the loop given {samples, valid, unobserved + outside}; what
 *             ends where is the same.  res->T is camera-to-world.
 * Legality and refusals, in this order: a null argument (opt and res may be null) or an option that is negative or not finite,
 * DR_ERR_ARG naming the option; not where drf_integrate_scan_async is legal, DR_ERR_PROTOCOL; a pose that drf_transform_map would
 * refuse, DR_ERR_ARG; in DRF_LOCATE_MAP a selection above the staging's capacity, DR_ERR_CAPACITY.  DR_OK means the call ran: a
 * refinement that ends DRF_ALIGN_DEGENERATE or DRF_ALIGN_LOST returns DR_OK with res->status set and a message in dr_last_error()
 * (in DRF_LOCATE_MAP it says how many of the stored blocks were staged). */
typedef struct {
  int    max_iters;     /* 0 -> 30 */
  int    min_weight;    /* 0 -> 1; a voxel counts as observed iff weight >= min_weight */
  int    step;          /* pixel stride of the sample grid; 0 -> 1 */
  float  band;          /* metres; 0 -> truncation_distance; samples with |phi| < band are used */
  float  huber;         /* voxels; 0 -> 1.0 */
  float  centre_depth;  /* metres; the centre of rotation lies this far along the optical axis; 0 = the camera centre */
  double eps_rot;       /* rad; 0 -> 1e-7 */
  double eps_trans;     /* voxels; 0 -> 1e-5 */
  double min_valid;     /* share of the samples that must be valid; 0 -> 0.25 */
} drf_locate_options_t;
/* the system at pose16: sums[28] and counts = {samples, valid, unobserved, outside} */
int drf_locate_system(drf_t *h, const float *depth, const float pose16[16], const drf_locate_options_t *opt, double sums[28], uint64_t counts[4]);
/* the refinement from pose_init16; pose16_out = res->T rounded to float */
int drf_locate_frame(drf_t *h, const float *depth, const float pose_init16[16], const drf_locate_options_t *opt, float pose16_out[16],
                     drf_align_result_t *res);
/* the same with depth in device memory */
int drf_locate_system_device(drf_t *h, const void *d_depth, const float pose16[16], const drf_locate_options_t *opt, double sums[28],
                             uint64_t counts[4]);
int drf_locate_frame_device(drf_t *h, const void *d_depth, const float pose_init16[16], const drf_locate_options_t *opt, float pose16_out[16],
                            drf_align_result_t *res);
/* last drf_locate_*: [0] grid positions, [1] samples, [2] valid samples at the last evaluation, [3] system evaluations, [4] device
 * bytes held during the call, [5] blocks in the host store at the call (all 0 after a call that was refused) */
int drf_locate_stats(drf_t *h, uint64_t out[6]);
/* What drf_locate_* read (SCOPE above).  Unknown scope: DR_ERR_ARG; between RenderAsync and GetRenderResult: DR_ERR_PROTOCOL, as for
 * drf_set_render_scope (the two share the staging). */
#define DRF_LOCATE_RESIDENT 0   /* default */
#define DRF_LOCATE_MAP      1
int drf_set_locate_scope(drf_t *h, int scope, size_t stage_capacity_blocks);
/* last drf_locate_*: [0] stagings made, [1] blocks in the largest staging, [2] blocks staged in total, [3] evaluations that read a
 * staging (all 0 in resident scope, with nothing to stage, or after a call that was refused) */
int drf_locate_stage_stats(drf_t *h, uint64_t out[4]);
/* Tracks a depth frame against the ray-cast model of the map the engine holds (DESIGN.md §7c "Tracking a depth frame against the
 * ray-cast model"): the classical frame-to-model step, projective data association and point-to-plane Gauss-Newton.  Where
 * drf_locate_frame needs a start inside the truncation band (a few centimetres), this call's basin is set by the association:
 * decimetres and some ten degrees.  It ends close enough for drf_locate_frame to do the sub-voxel part -- the ray-cast stops up to
 * one voxel in front of the surface, so this call alone is good to about a voxel.  From a rough pose: drf_track_frame, then
 * drf_locate_frame from the pose it returns.  Out of scope: a global search, a test that compares
 * the frame's own normals with the model's; for an image pyramid call drf_track_pyramid_frame.  With the frame's colour image at hand call
 * drf_track_colour_frame, below: its photometric term holds the motion inside a plane, which this call leaves open.
 * drf_track_frame renders the map at the current estimate into buffers of its own -- the engine's ray-cast, under
 * drf_set_render_scope and drf_set_render_bands as drf_render_async plans it (DRF_RENDER_MAP reads the host store too, and a
 * selection above the staging is DR_ERR_CAPACITY in the same way) -- builds the model map, runs a few evaluations against it and
 * renders again.  The public render buffers, drf_get_render_device and the render protocol are not touched; the map is neither
 * changed nor grown.  The call runs on the integration stream behind any pending scan and returns when it is done.
 * drf_track_system is one evaluation against a model depth image the caller supplies (a ray-cast at model_pose16): it reads no map.
 * The rule (one text, pose_host.h, compiled for the host and for the kernels; double and fp32 without contraction; only + - * /
 * sqrt and floor are used):
 *   model map Per pixel (u, v) of the model depth image Dm (height x width floats, a ray-cast at the pose Pm) four fp32 values
 *             (nx, ny, nz, z), all 0 where the pixel is INVALID.  A miss of the ray-cast is the 0.0f it writes for a ray that found
 *             no surface; the test is !(z > 0), which a NaN and a negative value fail too.  Invalid: the pixel is a miss; it lies
 *             on the image border (u = 0, v = 0, u = width - 1 or v = height - 1); one of its neighbours (u - 1, v), (u + 1, v),
 *             (u, v - 1), (u, v + 1) is a miss; or |z_neighbour - z| > max_jump for one of them (fp32 subtraction and compare: a
 *             depth discontinuity).  Otherwise, in fp32, X(u, v, z) = ((((float)u - cx) / fx) * z, (((float)v - cy) / fy) * z, z),
 *             a = X(u + 1, v, Dm(u + 1, v)) - X(u - 1, v, Dm(u - 1, v)), b = X(u, v + 1, ..) - X(u, v - 1, ..) (each component
 *             the difference of the two products), n = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0),
 *             l2 = (n0 n0 + n1 n1) + n2 n2; !(l2 > 0) is invalid; n = n / sqrt(l2) component by component; and with
 *             s = (n0 X0 + n1 X1) + n2 X2 at the centre pixel, s > 0 negates n, so that the normal looks at the camera.
 *             z = Dm(u, v).
 *   sample    drf_locate_*'s grid, test and point: grid position n = j * Wg + i with pixel stride step, a SAMPLE iff dep > 0,
 *             dep >= min_sensor_depth and dep <= max_sensor_depth in fp32; g in double as there; q = Rd g + tv at the estimate.
 *   association  in double.  (Rm, tvm) = model_pose16 as a pose is read above.  s = q - tvm, m_k = (Rm[0][k] s0 + Rm[1][k] s1) +
 *             Rm[2][k] s2: the point in the model camera.  !(m2 > 0) is UNASSOCIATED.  u' = (double)fx * (m0 / m2) + (double)cx,
 *             v' = (double)fy * (m1 / m2) + (double)cy, pu = floor(u' + 0.5), pv = floor(v' + 0.5); outside 0 <= pu <= width - 1,
 *             0 <= pv <= height - 1, or at an invalid model pixel, is UNASSOCIATED.  z = (double)(the pixel's z),
 *             vm = ((((pu - cx) / fx) * z) / vs, (((pv - cy) / fy) * z) / vs, z / vs), d = m - vm.  If
 *             (d0 d0 + d1 d1) + d2 d2 <= lim * lim is false, lim = (double)dist_max / vs, the sample is REJECTED.
 *   residual  n = the pixel's normal widened to double; r = (n0 d0 + n1 d1) + n2 d2, the point-to-plane distance in voxels;
 *             nw_k = (Rm[k][0] n0 + Rm[k][1] n1) + Rm[k][2] n2; x = q - c; J = (x cross nw, nw).  From here Huber's weight and the
 *             28 sums are drf_align_map's.  centre: drf_locate_*'s (centre_depth).
 *   order     drf_locate_*'s groups, lanes, butterfly and fold.  counts = {samples, valid, unassociated, rejected}.
 *   step, loop, statuses: drf_align_map's, the loop given {samples, valid, unassociated + rejected}.
 *   outer loop  p16 = pose_init16.  A round renders the model at p16, builds the model map and runs the loop from that very pose
 *             (Rd, tv read from p16; Pm = p16) for at most inner_iters evaluations.  A round that ends DRF_ALIGN_LOST or
 *             DRF_ALIGN_DEGENERATE ends the call with that status, what ends where as for drf_locate_frame; a round that
 *             converges at its first evaluation ends the call DRF_ALIGN_CONVERGED; after any other round p16 = the round's T
 *             rounded to float (what a drf_render_async at that pose16 renders, bit for bit), and after max_renders rounds the
 *             call is DRF_ALIGN_MAX_ITERS.  res: T, sums, samples, valid, cost of the last round, valid0 and cost0 of the
 *             first, iterations = the evaluations of all rounds.
 * Legality and refusals, in drf_locate_frame's order: a null argument (opt and res may be null) or an option that is negative or
 * not finite, DR_ERR_ARG naming it; not where drf_integrate_scan_async is legal, DR_ERR_PROTOCOL; a pose (or model pose) that
 * drf_transform_map would refuse, DR_ERR_ARG; the render's DR_ERR_CAPACITY.  drf_track_stats is all zero after a refused call.
 * DR_OK means the call ran: DRF_ALIGN_DEGENERATE or DRF_ALIGN_LOST return DR_OK with res->status set and a message in
 * dr_last_error().  Device memory is sized once per engine: 16 W H (model map) + 4 W H (model depth) + 4 W H (the frame) bytes, the
 * groups' partial sums and 64 bytes of counters. */
typedef struct {
  int    max_renders;   /* 0 -> 10 */
  int    inner_iters;   /* evaluations per render; 0 -> 4 */
  int    step;          /* pixel stride of the sample grid; 0 -> 1 */
  float  dist_max;      /* metres; 0 -> 25 * voxel_size; a sample farther than this from its model vertex is rejected */
  float  max_jump;      /* metres; 0 -> 5 * voxel_size; neighbouring model depths that differ by more are a discontinuity */
  float  huber;         /* voxels; 0 -> 1.0 */
  float  centre_depth;  /* metres, as in drf_locate_options_t */
  double eps_rot;       /* rad; 0 -> 1e-7 */
  double eps_trans;     /* voxels; 0 -> 1e-5 */
  double min_valid;     /* share of the samples that must be valid; 0 -> 0.25 */
} drf_track_options_t;
/* one evaluation at pose16 against the model depth ray-cast at model_pose16: sums[28], counts = {samples, valid, unassociated, rejected} */
int drf_track_system(drf_t *h, const float *depth, const float *model_depth, const float model_pose16[16], const float pose16[16],
                     const drf_track_options_t *opt, double sums[28], uint64_t counts[4]);
/* the tracking from pose_init16; pose16_out = res->T rounded to float */
int drf_track_frame(drf_t *h, const float *depth, const float pose_init16[16], const drf_track_options_t *opt, float pose16_out[16],
                    drf_align_result_t *res);
/* the same with the images in device memory */
int drf_track_system_device(drf_t *h, const void *d_depth, const void *d_model_depth, const float model_pose16[16], const float pose16[16],
                            const drf_track_options_t *opt, double sums[28], uint64_t counts[4]);
int drf_track_frame_device(drf_t *h, const void *d_depth, const float pose_init16[16], const drf_track_options_t *opt, float pose16_out[16],
                           drf_align_result_t *res);
/* last drf_track_*: [0] grid positions, [1] samples, [2] valid samples at the last evaluation, [3] system evaluations, [4] renders,
 * [5] device bytes held (all 0 after a call that was refused) */
int drf_track_stats(drf_t *h, uint64_t out[6]);
/* Tracks a depth frame AND its colour image against the ray-cast model (DESIGN.md §7c "Tracking with colour").  drf_track_frame
 * sees geometry only: on a map of planes -- most indoor maps -- the motion inside the planes is open, and on one plane the call is
 * DRF_ALIGN_DEGENERATE.  Every voxel carries a colour and the ray-cast renders it, so these calls add, for every sample whose
 * geometric term was added, a photometric term: the model's colour image, interpolated where the sample projects, against the
 * frame's own pixel.  bgr is the frame's colour image as drf_integrate_scan_async takes it (height x width x 3 bytes, B G R),
 * model_bgr the ray-cast's at model_pose16.  Everything that drf_track_* say above about the render, its scope and bands, the
 * stream, the map left unchanged, the legality and the refusals (in that order, the colour images among the null checks) holds
 * here.  Frame and map are taken to share their exposure: a frame whose exposure differs is drf_track_exposure_frame's, below.
 * Out of scope: a global search, and photometric terms in drf_locate_*; the image pyramid is drf_track_pyramid_frame, below.
 * The rule (the same text of pose_host.h; double and fp32 without contraction; + - * / sqrt floor):
 *   intensity   a BGR pixel is y = ((float)b + (float)g) + (float)r, a whole number in 0..765.
 *   Ym          the model intensity map, one float per pixel of the model colour image Cm: Ym(u, v) = the pixel's y where the model
 *               map's pixel is valid (its z > 0), -1.0f elsewhere: misses, the border and depth discontinuities carry no colour.
 *   sample, association, geometric term: drf_track_*'s, unchanged, and added FIRST.  The photometric term is attempted only for a
 *               sample whose geometric term was added, so the dist_max test is its occlusion test.
 *   photometric term  in double, from the m, u', v' of the association.  u0 = floor(u'), v0 = floor(v'), a = u' - u0, b = v' - v0.
 *               The term is SKIPPED unless 0 <= u0, u0 + 1 <= width - 1, 0 <= v0, v0 + 1 <= height - 1 and y00 = Ym(u0, v0),
 *               y10 = Ym(u0 + 1, v0), y01 = Ym(u0, v0 + 1), y11 = Ym(u0 + 1, v0 + 1) (each widened to double) are all >= 0.
 *               oa = 1 - a, ob = 1 - b;
 *               I  = ob * (oa * y00 + a * y10) + b * (oa * y01 + a * y11);
 *               Iu = ob * (y10 - y00) + b * (y11 - y01), Iv = oa * (y01 - y00) + a * (y11 - y10): the exact gradient of I;
 *               gm0 = (Iu * (double)fx) / m2, gm1 = (Iv * (double)fy) / m2, gm2 = -((gm0 * m0 + gm1 * m1) / m2);
 *               lambda = (double)photo_weight, yf = the intensity of the frame's pixel at the sample's own (u, v):
 *               r = lambda * (I - (double)yf), n_k = lambda * ((Rm[k][0] gm0 + Rm[k][1] gm1) + Rm[k][2] gm2).
 *               From (r, n) on the term is a sample of drf_align_map's like the geometric one: J = ((q - c) cross n, n), Huber's
 *               weight on |r| (in voxels after the scaling), the same 28 sums, the geometric term's additions before it.
 *   counts      {samples, valid, unassociated, rejected, photometric terms added}; the loop is given {samples, valid,
 *               unassociated + rejected}.  res->cost = sums[27] / valid carries BOTH terms.
 *   order, step, loop, statuses, outer loop: drf_track_*'s. */
typedef struct {
  drf_track_options_t track;
  float photo_weight;   /* voxels per intensity unit; 0 -> (float)(1.0 / 27.0) * huber (fp32, huber resolved first): 27 units of the
                           three-channel sum, 9 grey levels of 255, weigh what a geometric residual at Huber's threshold weighs */
} drf_track_colour_options_t;
/* one evaluation at pose16 against the model colour and depth ray-cast at model_pose16: sums[28], counts[5] as above */
int drf_track_colour_system(drf_t *h, const uint8_t *bgr, const float *depth, const uint8_t *model_bgr, const float *model_depth,
                            const float model_pose16[16], const float pose16[16], const drf_track_colour_options_t *opt, double sums[28], uint64_t counts[5]);
/* the tracking from pose_init16; pose16_out = res->T rounded to float */
int drf_track_colour_frame(drf_t *h, const uint8_t *bgr, const float *depth, const float pose_init16[16], const drf_track_colour_options_t *opt,
                           float pose16_out[16], drf_align_result_t *res);
/* the same with the images in device memory */
int drf_track_colour_system_device(drf_t *h, const void *d_bgr, const void *d_depth, const void *d_model_bgr, const void *d_model_depth,
                                   const float model_pose16[16], const float pose16[16], const drf_track_colour_options_t *opt, double sums[28],
                                   uint64_t counts[5]);
int drf_track_colour_frame_device(drf_t *h, const void *d_bgr, const void *d_depth, const float pose_init16[16], const drf_track_colour_options_t *opt,
                                  float pose16_out[16], drf_align_result_t *res);
/* last drf_track_colour_*: drf_track_stats' fields.  [5]: a buffer of these calls' own, sized once per engine at the first of them
 * (the partial sums, 64 bytes of counters, 16 W H model map, 4 W H model depth, 3 W H model colour, 4 W H Ym, 4 W H + 3 W H for a
 * frame given by host pointer); drf_track_stats()[5] does not change. */
int drf_track_colour_stats(drf_t *h, uint64_t out[6]);
/* Tracks a frame coarse to fine, over an image pyramid (no reference counterpart; DESIGN.md §7c "Tracking coarse to fine").
 * drf_track_frame and drf_track_colour_frame run at the camera's resolution: where the map's texture is finer than a rendered pixel
 * the render aliases it and the cost has minima at the texture's scale.  These calls run the same rule on images halved L times,
 * level L = levels - 1 down to 0, each level from the pose the one above ended on.  The pyramid is a cure for aliasing and for
 * texture-scale local minima; it is NOT a global search: a start whose samples fall outside the model is DRF_ALIGN_LOST at every
 * level.  Track with the pyramid, then drf_locate_frame from the pose it returns.  bgr null: geometry only (drf_track_frame's rule
 * at every level).  The rule (the same text of pose_host.h; fp32 without contraction; + - * / sqrt floor and integers):
 *   level       s = 2^L.  W_L = W / s, H_L = H / s by integer division: remainder columns and rows are dropped.  In fp32
 *               fx_L = fx / s, fy_L = fy / s, cx_L = (cx + 0.5f) / s - 0.5f, cy_L likewise; level 0 is the camera itself.  step, the
 *               sensor depth limits, dist_max, huber, photo_weight, min_valid and the epsilons are unchanged;
 *               max_jump_L = (float)s * max_jump, max_jump resolved first.  A level with W_L < 8 or H_L < 8 is refused, as is
 *               levels > 5.
 *   reduction   of a (bgr, depth) pair to level L, the same for frame and model.  Level pixel (u, v) covers the block
 *               [u s, u s + s) x [v s, v s + s).  A pixel is VALID iff z > 0 in fp32 (a NaN is not).  z0 = the smallest valid depth
 *               of the block; none: depth 0.0f, colour 0, 0, 0.  A pixel is ACCEPTED iff it is valid and z - z0 <= max_jump_L in
 *               fp32; n = the accepted pixels.  2 n < s s: depth 0.0f, colour 0, 0, 0.  Otherwise depth = S / (float)n: a pixel that
 *               is not accepted contributes +0.0f; each row of the block is summed by the butterfly t[i] = t[i] + t[i ^ off] for
 *               off = s / 2 .. 1, the row's sum is t[0]; the rows are added in ascending order from the first row's sum.  Per
 *               channel, c = the integer sum over the accepted pixels, the output is (2 c + n) / (2 n) by integer division (half up).
 *   evaluation  drf_track_colour_*'s rule (drf_track_*'s without colour) on the reduced images with the level's camera.
 *   schedule    The frame is reduced once per call to every level >= 1.  For L = levels - 1 down to 1 the outer loop of drf_track_*
 *               runs at level L with max_renders = coarse_renders; a round renders the model at FULL resolution (the engine's one
 *               submit: bit for bit a drf_render_async at that pose), reduces it to level L, builds the model map (and Ym) and
 *               evaluates.  A level that ends DRF_ALIGN_LOST or DRF_ALIGN_DEGENERATE is ABANDONED: the pose it started from goes to
 *               the next finer level.  Any other level hands on its T rounded to float.  Level 0 is then the existing call's loop
 *               from that pose with max_renders as given, and res is level 0's result, exactly: levels = 1 is
 *               drf_track_colour_frame, with bgr null drf_track_frame, bit for bit.
 * drf_track_reduce is the reduction alone: full-resolution images in, W_L x H_L images out; max_jump is the level's own (not scaled
 * again; it must be finite and >= 0); bgr null reduces the depth alone (bgr_out is not written).  drf_track_pyramid_system is one
 * evaluation at `level`: both pairs are given at full resolution and reduced first; counts[4] is 0 without colour.
 * Legality and refusals in drf_track_colour_frame's order, levels and coarse_renders among the options (after the colour options'
 * own): DR_ERR_ARG naming the option for a negative value, levels > 5 and a level below 8 pixels; `level` of drf_track_reduce and
 * drf_track_pyramid_system is judged with the options.  All statistics are zero after a refusal.  The render's DR_ERR_CAPACITY, its
 * scope and bands are as for drf_track_frame.  The public render buffers, drf_track_stats, drf_track_colour_stats and the map are
 * untouched: these calls have a scratch buffer of their own, sized once per engine for five levels. */
typedef struct {
  drf_track_colour_options_t colour;
  int levels;           /* 0 -> 3 */
  int coarse_renders;   /* renders per level above 0; 0 -> 3 */
} drf_track_pyramid_options_t;
int drf_track_reduce(drf_t *h, int level, float max_jump, const uint8_t *bgr, const float *depth, uint8_t *bgr_out, float *depth_out);
int drf_track_pyramid_system(drf_t *h, int level, const uint8_t *bgr, const float *depth, const uint8_t *model_bgr, const float *model_depth,
                             const float model_pose16[16], const float pose16[16], const drf_track_pyramid_options_t *opt, double sums[28], uint64_t counts[5]);
int drf_track_pyramid_frame(drf_t *h, const uint8_t *bgr, const float *depth, const float pose_init16[16], const drf_track_pyramid_options_t *opt,
                            float pose16_out[16], drf_align_result_t *res);
/* the same with every image, the outputs of the reduction included, in device memory */
int drf_track_reduce_device(drf_t *h, int level, float max_jump, const void *d_bgr, const void *d_depth, void *d_bgr_out, void *d_depth_out);
int drf_track_pyramid_system_device(drf_t *h, int level, const void *d_bgr, const void *d_depth, const void *d_model_bgr, const void *d_model_depth,
                                    const float model_pose16[16], const float pose16[16], const drf_track_pyramid_options_t *opt, double sums[28],
                                    uint64_t counts[5]);
int drf_track_pyramid_frame_device(drf_t *h, const void *d_bgr, const void *d_depth, const float pose_init16[16], const drf_track_pyramid_options_t *opt,
                                   float pose16_out[16], drf_align_result_t *res);
/* last drf_track_pyramid_* / drf_track_reduce: [0] grid positions, [1] samples and [2] valid samples at a level's last evaluation,
 * each summed over the levels that ran; [3] evaluations and [4] renders in all; [5] device bytes held; [6] levels run; [7] levels
 * abandoned (all 0 after a call that was refused; after drf_track_reduce only [5] is set) */
int drf_track_pyramid_stats(drf_t *h, uint64_t out[8]);
/* level 0 .. 4 of the last drf_track_pyramid_frame: [0] its status, [1] renders, [2] evaluations, [3] valid samples at its last
 * evaluation; all 0 for a level that did not run ([2] = 0 says so).  After drf_track_pyramid_system: the one evaluation at its level. */
int drf_track_pyramid_level_stats(drf_t *h, int level, uint64_t out[4]);
/* Tracks a frame whose exposure differs from the map's (the counterpart of the two affine brightness parameters the reference's
 * CoarseTracker / cuda_coarse_tracker solves next to its pose; DESIGN.md §7c "Tracking under a change of exposure").  Every colour
 * call above takes frame and map to share their exposure.  A camera changes it from frame to frame, and where geometry says nothing
 * -- one wall, a corridor: what the colour term is for -- a brightness change then puts the pose in the wrong place, with no status
 * that says so.  These calls are drf_track_pyramid_* with colour (bgr is required) and two more unknowns in the solver's state:
 * frame intensity ~ G * (model intensity) + B, gain G and offset B in double, B in units of the intensity (the three-channel sum
 * 0..765).  The rule (the same text of pose_host.h; double without contraction; + - * / sqrt floor, no exp):
 *   sample, association, geometric term   drf_track_*'s, unchanged, added FIRST, and to the 28 pose sums only.
 *   photometric term   from drf_track_colour_*'s I and gm (its conditions, unchanged) and the frame's yf:
 *               r = lambda * ((G * I + B) - (double)yf), n_k = (lambda * ((Rm[k][0] gm0 + Rm[k][1] gm1) + Rm[k][2] gm2)) * G;
 *               G = 1, B = 0 gives drf_track_colour_*'s bits.  J = ((q - c) cross n, n) and Huber's weight w on |r| as there, the
 *               28 pose sums as there; J6 = lambda * I (dr/dG), J7 = lambda (dr/dB), and 17 more sums, each (w * J_a) * J_b or
 *               (w * J_a) * r: H(i,6) for i = 0..5, H(i,7) for i = 0..5, H66, H67, H77, b6, b7.
 *   sums[45]    [0..27] the pose system in drf_track_colour_system's layout, [27] the cost of both terms; [28..44] the 17 above.
 *               counts[5] are drf_track_colour_system's.  Groups, lanes, butterfly and fold are drf_track_colour_system's.
 *   step        the 8 x 8 system solved by drf_align_map's Cholesky, its pivot test p > 1e-12 top with top over the 8 diagonals.  A
 *               failing pivot 0..5 is DRF_ALIGN_DEGENERATE.  A failing pivot 6 or 7 HOLDS the exposure (a map of one colour, no
 *               photometric term): the step is drf_track_*'s own on sums[0..27], G and B keep their values, `held` goes up.
 *               Otherwise a NaN in d is DEGENERATE; CONVERGED (not applied) needs the rotation and translation below eps_rot and
 *               eps_trans, |d6| < eps_gain and |d7| < eps_offset; any other step moves the pose as drf_align_map's does and sets
 *               G = min(max(G + d6, gain_min), gain_max), B = min(max(B + d7, -765), 765).  The gain is bounded because an
 *               unbounded one can go negative from a far start (contrast inversion) and end tens of voxels off.
 *   loop        drf_track_pyramid_frame's, with (G, B) part of the state: LOST restores the last good pose and exposure; the
 *               exposure carries from round to round and from level to level; an abandoned level hands on the pose and the
 *               exposure it started from; level 0's result is the call's.
 * Legality, the call order, render scope and bands, DR_ERR_CAPACITY and the note after a tracking that ran but found no pose are
 * drf_track_pyramid_frame's; level 0 is the camera itself and fits a camera of any size, as for drf_track_colour_*: levels = 1 is
 * not refused below 8 pixels on a side, nor is level 0 of drf_track_exposure_system.  Refusals in the pyramid options' order, then (DR_ERR_ARG naming the option) gain_init, offset_init,
 * gain_min, gain_max, eps_gain, eps_offset negative (not offset_init) or not finite; gain_min > gain_max; gain_init outside the
 * bounds; |offset_init| > 765; a null bgr is DR_ERR_ARG among the null arguments.  The public render buffers, the map, the
 * streaming state and the other families' statistics and buffers are untouched: these calls have a scratch buffer of their own
 * (the pyramid's layout with 45 doubles per group of 512 grid positions), sized once per engine.
 * OUT OF SCOPE: exposure in drf_score_colour_poses and in drf_locate_*; the tracking stage of drf_search_colour_frame, which keeps
 * calling the pyramid rule; per-channel gains, response curves and vignetting; compensation on the device (the frame is
 * compensated on the host before it is integrated: INTEGRATION.md, compensate_exposure). */
typedef struct {
  drf_track_pyramid_options_t pyramid;
  float gain_init;      /* 0 -> 1 */
  float offset_init;    /* used as given; |offset_init| <= 765 */
  float gain_min;       /* 0 -> 0.25 */
  float gain_max;       /* 0 -> 4 */
  double eps_gain;      /* 0 -> 1e-4 */
  double eps_offset;    /* 0 -> 1e-2 (intensity units) */
} drf_track_exposure_options_t;
typedef struct {
  drf_align_result_t pose;  /* level 0's result, as drf_track_pyramid_frame's */
  double gain, offset;      /* the exposure the call ended on */
  double ext[17];           /* sums[28..44] of the last evaluation */
  uint64_t photometric;     /* photometric terms added at the last evaluation */
  uint64_t held;            /* evaluations, over all levels, whose step held the exposure */
} drf_exposure_result_t;
/* one evaluation at `level`, pose16 and the exposure (gain, offset) against the model pair ray-cast at model_pose16 */
int drf_track_exposure_system(drf_t *h, int level, const uint8_t *bgr, const float *depth, const uint8_t *model_bgr, const float *model_depth,
                              const float model_pose16[16], const float pose16[16], double gain, double offset, const drf_track_exposure_options_t *opt,
                              double sums[45], uint64_t counts[5]);
/* the tracking from pose_init16 and (gain_init, offset_init); pose16_out = res->pose.T rounded to float */
int drf_track_exposure_frame(drf_t *h, const uint8_t *bgr, const float *depth, const float pose_init16[16], const drf_track_exposure_options_t *opt,
                             float pose16_out[16], drf_exposure_result_t *res);
/* the same with the images in device memory */
int drf_track_exposure_system_device(drf_t *h, int level, const void *d_bgr, const void *d_depth, const void *d_model_bgr, const void *d_model_depth,
                                     const float model_pose16[16], const float pose16[16], double gain, double offset, const drf_track_exposure_options_t *opt,
                                     double sums[45], uint64_t counts[5]);
int drf_track_exposure_frame_device(drf_t *h, const void *d_bgr, const void *d_depth, const float pose_init16[16], const drf_track_exposure_options_t *opt,
                                    float pose16_out[16], drf_exposure_result_t *res);
/* last drf_track_exposure_*: drf_track_pyramid_stats' fields.  [5]: the bytes of these calls' own buffer, with n = width * height,
 * g = ceil(n / 512), n_L = max(1, (width >> L) * (height >> L)), the spans laid one behind the other, each at the alignment of its
 * element (the model map at 32 bytes, the ray state at 8): 360 g partial sums, 48 of counters, 4 of the ray-cast's flag, 16 n model
 * map, 8 n ray state, 4 n model depth, 4 n_1 its level, 4 n Ym, 4 n frame depth, 4 n_L for L = 1..4, 3 n model colour, 3 n_1 its
 * level, 3 n frame colour, 3 n_L for L = 1..4. */
int drf_track_exposure_stats(drf_t *h, uint64_t out[8]);
int drf_track_exposure_level_stats(drf_t *h, int level, uint64_t out[4]);
/* Finds a depth frame in the map from a lattice of poses (no reference counterpart; DESIGN.md §7c "Searching a pose lattice").  Every
 * call above refines and says so: a start further off needs a guess from elsewhere.  These calls make that guess when a session has
 * only a place-recognition hit, a stale key-frame pose or a lost tracker: drf_score_poses evaluates the localisation's cost, without
 * its Jacobian, at n poses of one depth image in one kernel (one wave per pose) instead of n drf_locate_system calls, and
 * drf_search_frame scores a lattice of poses around anchors, tracks the best few (drf_track_frame's rule), locates them
 * (drf_locate_frame's rule) and picks one.  It is a geometric score: it has no appearance term and is ambiguous where geometry
 * repeats (two alike corridors score alike) -- the runner-up entries of the result show it; drf_search_colour_frame, further below,
 * adds an appearance term from the voxel colours for frames that have a colour image.
 * SCOPE (drf_set_search_scope, below).  DRF_SEARCH_RESIDENT, the default: the score reads the resident map only: with streaming
 * on, blocks in the host store read as absent (their samples are UNOBSERVED) and drf_search_stats()[7] tells how many there are;
 * DRF_LOCATE_MAP does not apply to the score.  What applies is DRF_SEARCH_MAP: the score stage of all four calls and their _device
 * forms, the colour search's final re-score included, reads the pool and the host store together -- cost, photo, counts and score of
 * every candidate, all_scores, the selection and so the entries, the winner and the pose are, bit for bit, those of an engine whose
 * pool holds the whole map, whatever the split between pool and store, the staging's capacity and the chunking are.  No block
 * moves.  The host plans the table once (DESIGN.md §7c "Searching the whole map"): a run of candidates with one rotation whose
 * camera centres lie in a box is served by the render scope's selection at the box's centre, widened by the box's half-diagonal;
 * whole table entries first, halved along ix while a selection exceeds stage_capacity_blocks (0: min(num_blocks, 8192), the
 * render's default), neighbours merged while their union fits; each pass is staged once and scored in chunks.  A single ix-slab
 * of the lattice (a single pose of drf_score_poses) that can read more than the capacity: DR_ERR_CAPACITY before anything is
 * evaluated, naming both counts, drf_set_search_scope and drf_stream_in_region; nothing is written and all statistics are 0.
 * With an empty store or a pass that selects nothing the resident kernel runs and nothing is staged.  The refinement stages keep
 * their own scopes (drf_set_render_scope for the tracking's renders, drf_set_locate_scope for the localisation): a search of the
 * whole map wants all three set.  The map, the public render buffers and the streaming state are untouched; drf_track_stats,
 * drf_locate_stats and drf_locate_stage_stats afterwards describe the last refinement stage that ran.
 * The rule (one text, pose_host.h, compiled for the host and for the kernels; double and fp32 without contraction; + - * / floor):
 *   sample    drf_locate_*'s, to the letter: the grid of stride step, the sample test, the point g, q = Rd g + tv, b = floor(q),
 *             f = (float)(q - b), the eight voxels, UNOBSERVED (a corner of weight < min_weight, or q outside (-2^30, 2^30)), the
 *             trilinear fp32 phi, OUTSIDE (|phi| < band is false), r = (double)phi / vs, Huber's w = 1 if |r| <= huber else
 *             huber / |r|.  A valid sample adds (w r) r to one double; no gradient, no J and no centre exist.
 *   cost      the sum of (w r) r in drf_locate_system's order: groups of 512 grid positions, lane l of 64 on positions
 *             512 i + l + 64 k, k = 0..7, from +0.0; x = x + x[lane ^ off], off = 32 .. 1, gives partial[i]; lane i % 64 adds
 *             partial[i] in ascending i from +0.0 and the same butterfly folds the lanes.  For equal step, min_weight, band and
 *             huber, cost is bit for bit sums[27] of drf_locate_system at that float pose, and counts = {samples, valid,
 *             unobserved, outside} are its counts.
 *   score     ((cost + oc * (double)outside) + uc * (double)unobserved) / (double)samples, in double in that order; samples = 0
 *             gives uc.  LOWER IS BETTER.  oc = outside_cost, 0 -> (double)huber * ((double)band / vs), Huber's value at the band's
 *             edge; uc = unobserved_cost, 0 -> 2 oc.
 *   candidate (drf_search_frame) index c = (((a * n_rot + r) * Nx + ix) * Ny + iy) * Nz + iz, N = 2 half + 1.  The pose is formed on
 *             the host in double; no trigonometry runs anywhere in the library: rotations9 are n_rot row-major 3x3 matrices in
 *             double that the caller supplies.  (Ra, ta) = anchor a as every pose is read (ta = t / vs);
 *             Rd[i][j] = (Rr[i][0] Ra[0][j] + Rr[i][1] Ra[1][j]) + Rr[i][2] Ra[2][j], a turn about the WORLD axes through the camera
 *             centre; tv_k = ta_k + (double)(i_k - half_k) * ((double)trans_step / vs), offsets along the world axes.  The
 *             candidate's float pose is Rd and tv * vs rounded to float (what drf_locate_frame hands out).
 *   selection the top_k smallest scores, ties to the lower index (a NaN score ranks behind every number).
 *   refinement  each selected candidate in rank order: drf_track_frame's rule from its float pose with the track options; if that
 *             ends <= DRF_ALIGN_MAX_ITERS, drf_locate_frame's rule from the tracked pose16 with the locate options.  An entry
 *             QUALIFIES if its locate status is <= DRF_ALIGN_MAX_ITERS.  The winner has the greatest located valid among the
 *             qualifying, ties to the lower located cost, then to the better rank.  accept_valid > 0 ends the refinement at the
 *             first qualifying entry with valid >= accept_valid * samples, and that entry wins.  res->status is the winner's
 *             locate status and pose16_out its T rounded to float.  None qualifies: res->status = DRF_ALIGN_LOST, winner = -1,
 *             pose16_out is the best-scoring candidate's float pose, the return is DR_OK and dr_last_error() holds a message.
 *             score_only = 1: no refinement, winner = 0, status DRF_ALIGN_MAX_ITERS, pose16_out the best candidate's.
 *   steps     rule of thumb: trans_step about 2 * truncation_distance (the default), rotations about truncation_distance / scene
 *             depth apart (4 degrees at 8 cm and 1.2 m .. 2.3 m); DESIGN.md has the measurements behind it.
 * Candidates are scored in chunks: device scratch is the points (25 bytes per grid position), the pose table (96 bytes per anchor x
 * rotation, or per pose of a chunk) and 32 bytes per candidate of a chunk, whatever n is.
 * Legality and refusals, in drf_locate_frame's order: a null argument (the option structs, res, all_scores, and for drf_score_poses any
 * of the three outputs but not all, may be null); an option that is negative or not finite, a negative half, top_k >
 * DRF_SEARCH_MAX_TOP: DR_ERR_ARG naming it (the score and search options first, then the track, then the locate options); n = 0
 * or more than 2^24 candidates, DR_ERR_ARG; not where drf_integrate_scan_async is legal, DR_ERR_PROTOCOL; a pose, an anchor, a
 * rotation (taken as a pose without translation) or a product Rr Ra that drf_transform_map would refuse, DR_ERR_ARG naming its
 * index.  drf_search_stats is all zero after a refusal. */
#define DRF_SEARCH_MAX_TOP 32
typedef struct {
  int   step;             /* pixel stride of the sample grid; 0 -> 4 */
  int   min_weight;       /* 0 -> 1 */
  float band;             /* metres; 0 -> truncation_distance */
  float huber;            /* voxels; 0 -> 1.0 */
  float outside_cost;     /* voxels per OUTSIDE sample; 0 -> huber * band / voxel_size */
  float unobserved_cost;  /* voxels per UNOBSERVED sample; 0 -> 2 * outside_cost */
} drf_score_options_t;
/* n poses16 (n x 16 floats) scored against the resident map: cost[n], counts[n][4] = {samples, valid, unobserved, outside},
 * score[n]; each output may be null */
int drf_score_poses(drf_t *h, const float *depth, const float *poses16, size_t n, const drf_score_options_t *opt, double *cost, uint32_t *counts,
                    double *score);
int drf_score_poses_device(drf_t *h, const void *d_depth, const float *poses16, size_t n, const drf_score_options_t *opt, double *cost, uint32_t *counts,
                           double *score);
typedef struct {
  drf_score_options_t score;
  float  trans_step;    /* metres between neighbouring offsets; 0 -> 2 * truncation_distance */
  int    half[3];       /* offsets -half .. half along world x, y, z; 0 0 0: the anchors are turned, not moved */
  int    top_k;         /* candidates refined; 0 -> 8, at most DRF_SEARCH_MAX_TOP */
  int    score_only;    /* 1: no refinement */
  double accept_valid;  /* 0: refine all top_k; > 0: stop at the first entry whose located valid share reaches it */
} drf_search_options_t;
typedef struct {
  uint64_t index;                       /* the candidate */
  double   score, cost;                 /* of the score stage */
  uint32_t counts[4];
  int      track_status, locate_status; /* DRF_ALIGN_*; -1: the stage did not run */
  uint64_t samples, valid;              /* of the localisation's last evaluation (0 if it did not run) */
  double   located_cost;                /* its cost = sums[27] / valid */
  double   T[16];                       /* camera-to-world: the located pose, else the tracked pose, else the candidate's float pose */
} drf_search_entry_t;
typedef struct {
  int      status;                      /* DRF_ALIGN_*: the winner's locate status; DRF_ALIGN_LOST if no entry qualifies */
  int      n_entries;                   /* min(top_k, candidates) */
  int      winner;                      /* index into entries, -1: none */
  int      refined;                     /* entries whose refinement ran */
  uint64_t n_candidates;
  drf_search_entry_t entries[DRF_SEARCH_MAX_TOP];  /* in rank order: ascending score */
} drf_search_result_t;
/* the search around n_anchors poses (n_anchors x 16 floats) turned by n_rot rotations (n_rot x 9 doubles); all_scores, if given,
 * receives the score of every candidate in index order */
int drf_search_frame(drf_t *h, const float *depth, const float *anchors16, size_t n_anchors, const double *rotations9, size_t n_rot,
                     const drf_search_options_t *opt, const drf_track_options_t *track_opt, const drf_locate_options_t *locate_opt, float pose16_out[16],
                     drf_search_result_t *res, double *all_scores);
int drf_search_frame_device(drf_t *h, const void *d_depth, const float *anchors16, size_t n_anchors, const double *rotations9, size_t n_rot,
                            const drf_search_options_t *opt, const drf_track_options_t *track_opt, const drf_locate_options_t *locate_opt, float pose16_out[16],
                            drf_search_result_t *res, double *all_scores);
/* last drf_score_poses / drf_search_frame: [0] candidates, [1] grid positions, [2] samples, [3] chunks, [4] renders and [5] system
 * evaluations of the refinement, [6] device bytes held by the score stage, [7] blocks in the host store at the call (all 0 after a
 * call that was refused) */
int drf_search_stats(drf_t *h, uint64_t out[8]);
/* What the score stage of drf_score_poses, drf_score_colour_poses, drf_search_frame, drf_search_colour_frame and their _device forms
 * reads (SCOPE above).  Unknown scope: DR_ERR_ARG; between RenderAsync and GetRenderResult: DR_ERR_PROTOCOL, as for
 * drf_set_locate_scope (the render, the locate and the search scope share the staging, which holds the largest of their needs). */
#define DRF_SEARCH_RESIDENT 0   /* the default: today's behaviour, bit for bit */
#define DRF_SEARCH_MAP      1
int drf_set_search_scope(drf_t *h, int scope, size_t stage_capacity_blocks);
/* last search call of either family: [0] stagings made, [1] blocks in the largest staging, [2] blocks staged in total, [3] score
 * launches that read a staging, the final re-score's included (all 0 in resident scope, with nothing to stage, or after a call that
 * was refused) */
int drf_search_stage_stats(drf_t *h, uint64_t out[4]);
/* The search with an appearance term from the voxel colours (no reference counterpart; DESIGN.md §7c "Searching with colour").  The
 * score above is geometric, and it is ambiguous wherever geometry says nothing: on ONE wall every in-plane offset of the lattice
 * scores alike, and the winner is whatever the tie rule picks.  Every voxel carries a colour, and the score's fetch of a corner
 * already loads it; these calls keep it.  drf_score_colour_poses is drf_score_poses with a second sum, photo, and
 * drf_search_colour_frame is drf_search_frame selecting on the colour score, tracking with the frame's colour image and picking the
 * winner by the colour score of the located poses.  The geometric calls stay as they are, for frames without colour.
 * The rule (pose_host.h score_sample with colour, the one text the host and k_search_score_colour compile; + - * / floor):
 *   sample    drf_score_poses', to the letter, up to and including cost = cost + (w r) r.  A valid sample goes on:
 *   y[c]      ((float)c0 + (float)c1) + (float)c2 of corner c, c0, c1, c2 = bits 0-7, 8-15, 16-23 of the voxel's second word (its
 *             stored B, G, R): a whole number in 0..765, the intensity of drf_track_colour_*.
 *   Ym        the fp32 trilinear interpolant of y[] in phi's three stages and order (z, then y, then x) with the same f.
 *   yf        the same intensity of the frame's BGR pixel at the sample's own (u, v).
 *   term      rp = lambda * ((double)Ym - (double)yf), lambda = (double)photo_weight; wp = 1 if |rp| <= huber else huber / |rp|
 *             (the geometric huber); tp = (wp rp) rp, and tp = pc where tp > pc: a sample whose colour disagrees costs at most
 *             pc.  photo = photo + tp, after the geometric addition.
 *   photo     reduced exactly as cost is: per lane from +0.0, the group butterfly, lane i % 64 adds partial i in ascending i, the
 *             last butterfly.
 *   score     (((cost + photo) + oc * (double)outside) + uc * (double)unobserved) / (double)samples; samples = 0 gives uc.
 *   options   photo_weight 0 -> (float)(1.0 / 27.0) * huber in fp32, huber resolved first (drf_track_colour_options_t's default);
 *             photo_cap 0 -> oc.
 * Two invariants hold bit for bit: cost and counts equal drf_score_poses' at the same score options; on a map of one colour and
 * a frame image of that colour photo is +0.0 at every pose and score has drf_score_poses' bits.
 * drf_search_colour_frame: candidates, index order, the pose table and chunking are drf_search_frame's.  The selection takes the
 * top_k smallest COLOUR scores, ties to the lower index, a NaN last.  Each selected entry in rank order: drf_track_pyramid_frame's
 * rule with the frame's bgr from the candidate's float pose (track_opt null: its defaults; levels = 1: drf_track_colour_frame); if
 * that ends <= DRF_ALIGN_MAX_ITERS, drf_locate_frame's rule; an entry qualifies as in drf_search_frame.  When the refinement has
 * ended, the located float pose of every qualifying entry is scored once more by the colour score (one launch, in rank order):
 * final_score, final_photo (0 for an entry that does not qualify).  The winner has the smallest final_score among the qualifying,
 * ties to the better rank; accept_valid > 0 ends the refinement at the first qualifying entry that reaches the share, and that entry
 * wins.  score_only, the LOST convention and the statuses are drf_search_frame's.
 * Device scratch: drf_search_frame's plus 4 bytes per grid position (yf), a 40-byte record per candidate of a chunk (cost, photo,
 * counts[4], score) instead of 32, and a colour image (3 bytes per pixel) for a host-given frame.
 * SCOPE and side effects are drf_search_frame's: the resident map only by default, stored blocks counted in [7], and with
 * drf_set_search_scope(DRF_SEARCH_MAP) pool and host store together, the final re-score included; the map, the public render
 * buffers and the streaming state untouched; drf_track_pyramid_stats and drf_locate_stats describe the last refinement stage that
 * ran.  drf_search_stats describes the last call of either family; the final re-score is not counted in [0] or [3].
 * OUT OF SCOPE: exposure or affine brightness (frame and map share their exposure here; drf_track_exposure_frame solves for it, and
 * the tracking stage of this search keeps the pyramid rule); selection on the device, a coarse-to-fine lattice, rotations about the camera's own axes.
 * Legality and refusals follow drf_search_frame's order: a null argument (bgr among them: a null bgr is DR_ERR_ARG -- the
 * geometric call is for frames without colour; for drf_score_colour_poses any of the four outputs but not all may be null); the
 * score or search options, then photo_weight and photo_cap (negative or not finite), then the track, then the locate options; the
 * count of candidates; the call order; the poses by index. */
typedef struct {
  drf_score_options_t score;
  float photo_weight;  /* voxels per intensity unit; 0 -> (1 / 27) * huber */
  float photo_cap;     /* voxels^2: the most one sample's colour term adds; 0 -> outside_cost */
} drf_score_colour_options_t;
/* cost[n], photo[n], counts[n][4], score[n]; each output may be null, not all */
int drf_score_colour_poses(drf_t *h, const uint8_t *bgr, const float *depth, const float *poses16, size_t n, const drf_score_colour_options_t *opt, double *cost,
                           double *photo, uint32_t *counts, double *score);
int drf_score_colour_poses_device(drf_t *h, const void *d_bgr, const void *d_depth, const float *poses16, size_t n, const drf_score_colour_options_t *opt,
                                  double *cost, double *photo, uint32_t *counts, double *score);
typedef struct {
  drf_search_options_t search;
  float photo_weight;
  float photo_cap;
} drf_search_colour_options_t;
typedef struct {  /* drf_search_entry_t's fields, then the colour sums */
  uint64_t index;
  double   score, cost;                 /* of the score stage: the colour score, the geometric sum */
  uint32_t counts[4];
  int      track_status, locate_status;
  uint64_t samples, valid;
  double   located_cost;
  double   T[16];
  double   photo;                       /* of the score stage */
  double   final_score, final_photo;    /* the colour score of the located float pose (0: the entry did not qualify) */
} drf_search_colour_entry_t;
typedef struct {
  int      status;
  int      n_entries;
  int      winner;
  int      refined;
  uint64_t n_candidates;
  drf_search_colour_entry_t entries[DRF_SEARCH_MAX_TOP];  /* in rank order: ascending colour score */
} drf_search_colour_result_t;
int drf_search_colour_frame(drf_t *h, const uint8_t *bgr, const float *depth, const float *anchors16, size_t n_anchors, const double *rotations9, size_t n_rot,
                            const drf_search_colour_options_t *opt, const drf_track_pyramid_options_t *track_opt, const drf_locate_options_t *locate_opt,
                            float pose16_out[16], drf_search_colour_result_t *res, double *all_scores);
int drf_search_colour_frame_device(drf_t *h, const void *d_bgr, const void *d_depth, const float *anchors16, size_t n_anchors, const double *rotations9,
                                   size_t n_rot, const drf_search_colour_options_t *opt, const drf_track_pyramid_options_t *track_opt,
                                   const drf_locate_options_t *locate_opt, float pose16_out[16], drf_search_colour_result_t *res, double *all_scores);

/* --- incremental mesh: an extraction that returns only the blocks whose triangles may have changed (no reference counterpart;
 * DESIGN.md §7c "Incremental mesh", INTEGRATION.md "Incremental mesh").
 * The engine keeps a BASELINE: the box of the last update that was fetched and the scans integrated since that update was
 * launched.  An update over [lower, upper] returns PATCHES in ascending packed-key order (x, then y, then z, each biased by
 * 2^20: the block order of a full extraction): a block's coordinates and its triangles, exactly the rows drf_extract_mesh_async
 * + drf_get_mesh_sync over the same box emit for that block, in the same order.  A block is listed whenever its triangles MAY
 * differ from what the earlier updates of this baseline described (listed with zero triangles: it has none now); a block that
 * is not listed has not changed.  A consumer that keeps {block -> rows}, replaces the entry of every listed block and
 * concatenates its entries in ascending key order holds, byte for byte, the full extraction over that box at that moment.
 * An update is FULL -- every block of the scope is listed, the consumer starts from an empty store -- when it is the first,
 * when its box differs from the baseline's (the six floats compared bitwise), after drf_mesh_update_reset, after more than
 * DRF_MESH_UPDATE_MAX_SCANS scans since the previous update was launched (the drf_bench_* loops record their scans like
 * drf_integrate_scan_async and drf_integrate_device do), after a scan whose pose is not a finite rigid motion, and after a scan
 * that reported round-trip voxel mismatches (drf_stats [3]).  An update launched with no scan since the previous one lists
 * nothing and launches no mesh kernel.
 * Which blocks: block b is listed iff, for one of the 27 blocks around it and the pose of one recorded scan, the integration's
 * visibility test holds (block origin in front of the camera, block centre projects into the image) and the block origin lies
 * within max_sensor_depth * rho + truncation_distance + (15 sqrt(3) + 1) voxel_size of the camera centre (rho as in
 * drf_streaming_min_radius): a superset of the blocks a scan can have written, widened by the neighbours a block's cells read.
 * Protocol: legal where drf_extract_mesh_async is; one extraction of either kind may be pending, and launching while one is
 * pending or fetching with the other kind's getter is DR_ERR_PROTOCOL with the state untouched.  drf_extract_mesh_async and
 * drf_save_mesh never move the baseline.  The baseline advances when drf_get_mesh_update_sync succeeds; DR_ERR_CAPACITY
 * (max_blocks or num_max too small, or above 20 M triangles) leaves the update pending and the baseline where it was.  Scans
 * integrated after the launch belong to the next update.
 * Scope follows drf_set_mesh_scope.  DRF_MESH_MAP: the patches describe resident and stored blocks together and equal an
 * unbounded engine's.  DRF_MESH_RESIDENT while the host store holds blocks: the launch is DR_ERR_PROTOCOL -- the resident view
 * changes by eviction alone, which an update does not track.  Like the map pass an update folds pending evictions first and is
 * otherwise read-only: pool, slot order, host store, streaming state and the counters stay as they were. */
#define DRF_MESH_UPDATE_MAX_SCANS 16
int drf_extract_mesh_update_async(drf_t *h, const float lower[3], const float upper[3]);
/* Size of the pending update (waits for it, does not consume it): listed blocks, triangles, full. */
int drf_mesh_update_size(drf_t *h, size_t *nblk, size_t *ntri, int *full);
/* coords: 3 per listed block (max_blocks blocks of room); first: max_blocks + 1 rows of room, block i owns triangles
 * [first[i], first[i + 1]) of vert / cols (laid out as drf_get_mesh_sync's; num_max vertices of room); *num = 3 * triangles. */
int drf_get_mesh_update_sync(drf_t *h, size_t max_blocks, size_t num_max, size_t *nblk, int32_t *coords, uint64_t *first, size_t *num,
                             float *vert, float *cols, int *full);
/* The next update is full. */
int drf_mesh_update_reset(drf_t *h);
/* Last update launched: [0] blocks in scope, [1] blocks meshed again (= listed), [2] scans folded in, [3] full. */
int drf_mesh_update_stats(drf_t *h, uint64_t out[4]);

/* ======================================================================================================
 * DrCoarseTracker -- the dense coarse tracker operator.  Replaces
 *   tandem/libdr/cuda_coarse_tracker/include/public/cuda_coarse_tracker.h   (class CudaCoarseTracker)
 * member for member (Eigen arguments become plain arrays: matrices row-major, double where the reference is), plus
 * the dense-depth hand-off of CoarseTracker::setCoarseTrackingRef (src/FullSystem/CoarseTracker.cpp:655-725).
 * ====================================================================================================== */
typedef struct drt_s drt_t;
/* CudaCoarseTracker(w, h, setting_huberTH, setting_coarseCutoffTH)            cuda_coarse_tracker.h:11, .cpp:63-69 */
int drt_create(int w, int h, float setting_huberTH, float setting_coarseCutoffTH, int device, drt_t **out);
void drt_destroy(drt_t *t);                                                   /* ~CudaCoarseTracker / free(), .cpp:142-199 */
/* setK(w, h, fx, fy, cx, cy): w, h must equal the constructor's               cuda_coarse_tracker.h:13, .cpp:358-372 */
int drt_set_k(drt_t *t, int w, int h, float fx, float fy, float cx, float cy);
/* init(n_max = 0 -> w*h); a second call is DR_ERR_PROTOCOL                      cuda_coarse_tracker.h:17, .cpp:101-140 */
int drt_init(drt_t *t, int n_max);
/* setReference(n, pc_u, pc_v, pc_idepth, pc_color, ref_exposure, ref_aff_g2l)  cuda_coarse_tracker.h:21, .cpp:71-89 */
int drt_set_reference(drt_t *t, int n, const float *pc_u, const float *pc_v, const float *pc_idepth, const float *pc_color,
                      float ref_exposure, const double ref_aff_g2l[2]);
/* setNew(dInew): 3*w*h floats, (I, dx, dy) interleaved per pixel                cuda_coarse_tracker.h:23, .cpp:91-94 */
int drt_set_new(drt_t *t, const float *dInew);
/* Vec6 calcRes(refToNew 4x4, new_exposure, aff_g2l, cutoffTH)                   cuda_coarse_tracker.h:25, .cpp:217-288
 * refToNew row-major.  out6 = the reference's Vec6 (E, numTermsInE, shiftT/num, 0, shiftRT/num, saturated/numTermsInE);
 * sums7 (may be NULL) = the 7 raw sums in the order of cuda_coarse_tracker_private.h:8-15. */
int drt_calc_res(drt_t *t, const double refToNew[16], float new_exposure, const double aff_g2l[2], float cutoffTH, double out6[6],
                 double sums7[7]);
/* calcG(H_out 8x8, b_out 8, new_exposure, aff_g2l)                              cuda_coarse_tracker.h:27, .cpp:290-356
 * Uses the warped buffers of the last calcRes.  H row-major, scaled as the reference; raw45 (may be NULL) = the 45
 * unscaled upper-triangular sums. */
int drt_calc_g(drt_t *t, double H_out[64], double b_out[8], float new_exposure, const double aff_g2l[2], double raw45[45]);
/* The dense-depth branch of CoarseTracker::setCoarseTrackingRef (CoarseTracker.cpp:655-725), on the device: forward-warp
 * `depth` (w*h, metres, <= 0 invalid; sampled every `step` pixels) with p' = KRKi * (x*d, y*d, d) + Kt into the tracker's
 * reference frame (z-buffer minimum), then append every pixel of rows/cols [2, size-2) that received a depth -- and has
 * idepth0 <= 0 unless dense_only -- as (x, y, 1/depth, dIp0[3*i]) after the current points, row-major.  KRKi (row-major)
 * and Kt are the caller's float products K*R*Ki and K*t (:672-673).  on_device != 0: depth / idepth0 / dIp0 are device
 * pointers (e.g. a DrFusion render left in HBM).  *n_out = new point count.  DR_ERR_CAPACITY above n_max. */
int drt_append_dense_reference(drt_t *t, const float *depth, const float KRKi[9], const float Kt[3], int step, int dense_only,
                               const float *idepth0, const float *dIp0, int on_device, int *n_out);
/* synchronize / startTiming / endTimingMilliseconds                              cuda_coarse_tracker.h:30-34 */
int drt_synchronize(drt_t *t);
int drt_start_timing(drt_t *t);
int drt_end_timing_ms(drt_t *t, float *ms);
/* --- introspection hooks (no reference counterpart) --- */
int drt_get_points(drt_t *t, float *pc_u, float *pc_v, float *pc_idepth, float *pc_color, int cap, int *n); /* arrays may be NULL */
int drt_get_warped(drt_t *t, int which, float *out, int cap); /* which: 0 u, 1 v, 2 dx, 3 dy, 4 idepth, 5 residual, 6 weight */
int drt_get_zbuffer(drt_t *t, float *out);                    /* w*h projected depths of the last append, -1 = empty */

#ifdef __cplusplus
}
#endif
#endif /* DR_MI355X_H */
