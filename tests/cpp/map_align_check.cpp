// C entry points over the registration half of tandem_amd/csrc/fusion_host.h for tests/test_map_align.py (plain g++, no HIP):
// ma_system, one evaluation of the system at a pose (align_system_host: the rule of drf_align_system run on the host), ma_align,
// the whole registration (align_maps_host: the CPU reference of drf_align_map) with the sums of every evaluation, and ma_options,
// what the call makes of a drf_align_options_t.
#include "../../tandem_amd/csrc/fusion_host.h"

extern "C" {

// 0 and the resolved options to out7 = {max_iters, min_weight, band, huber, eps_rot, eps_trans, min_valid}; 1: refused
int ma_options(const drf_align_options_t *opt, float vs, double out7[7]) {
  dr::AlignOpt o;
  if (dr::align_options(opt, vs, o)) return 1;
  out7[0] = o.max_iters; out7[1] = o.min_weight; out7[2] = o.band; out7[3] = o.huber; out7[4] = o.eps_rot; out7[5] = o.eps_trans; out7[6] = o.min_valid;
  return 0;
}
// the system at T16: source and reference as ascending keys and n x 4096 bytes; 1 if the options are refused
int ma_system(const unsigned long long *src_keys, const unsigned char *src_vox, size_t n_src, const unsigned long long *ref_keys, const unsigned char *ref_vox,
              size_t n_ref, const float *T16, float vs, const drf_align_options_t *opt, double sums[28], unsigned long long counts[3]) {
  dr::AlignOpt o;
  if (dr::align_options(opt, vs, o)) return 1;
  const std::vector<unsigned long long> sk(src_keys, src_keys + n_src), rk(ref_keys, ref_keys + n_ref);
  const dr::HostMapSource ref(rk, ref_vox);
  double c_src[3];
  dr::align_centre_src(sk, c_src);
  uint64_t c[3];
  dr::align_system_host(sk, src_vox, ref, dr::align_eval(dr::map_motion(T16, vs), c_src, o, vs), sums, c);
  counts[0] = c[0]; counts[1] = c[1]; counts[2] = c[2];
  return 0;
}
// the registration from T16; trace receives the sums of the first min(iterations, trace_cap) evaluations; 1 if the options are refused
int ma_align(const unsigned long long *src_keys, const unsigned char *src_vox, size_t n_src, const unsigned long long *ref_keys, const unsigned char *ref_vox,
             size_t n_ref, const float *T16, float vs, const drf_align_options_t *opt, drf_align_result_t *res, double *trace, size_t trace_cap) {
  dr::AlignOpt o;
  if (dr::align_options(opt, vs, o)) return 1;
  const std::vector<unsigned long long> sk(src_keys, src_keys + n_src), rk(ref_keys, ref_keys + n_ref);
  const dr::HostMapSource ref(rk, ref_vox);
  std::vector<std::array<double, 28>> tr;
  dr::align_maps_host(sk, src_vox, ref, dr::map_motion(T16, vs), o, vs, *res, &tr);
  for (size_t i = 0; i < tr.size() && i < trace_cap; ++i) memcpy(trace + 28 * i, tr[i].data(), 224);
  return 0;
}

}  // extern "C"
