// C entry points over the rigid-resample half of tandem_amd/csrc/fusion_host.h for tests/test_map_transform.py (plain g++, no
// HIP): transform_pose_fault (what drf_transform_map accepts), plan_transform (the candidate destination blocks) and
// transform_blocks, the rule of drf_transform_map (transform_voxel / transform_block) run on the host over those candidates.
#include "../../tandem_amd/csrc/fusion_host.h"

// A whole map through the rule: source keys (ascending) and voxels (n x 4096) -> the destination blocks that hold a weighted
// voxel, ascending.  counts[0] = candidates evaluated, [1] = voxels written with weight > 0, [2] = voxels refused.
static std::vector<unsigned long long> transform_blocks(const std::vector<unsigned long long> &keys, const uint8_t *vox, const dr::MapMotion &m,
                                                        std::vector<uint8_t> &out_vox, uint64_t counts[3]) {
  const dr::HostMapSource src(keys, vox);
  const std::vector<unsigned long long> cand = dr::plan_transform(keys, m);
  std::vector<unsigned long long> kept;
  uint64_t c2[2] = {0, 0};
  uint8_t block[4096];
  for (unsigned long long k : cand) {
    int blk[3]; dr::unpack_key_host(k, blk);
    if (!dr::transform_block(m, blk, src, block, c2)) continue;
    kept.push_back(k);
    out_vox.insert(out_vox.end(), block, block + 4096);
  }
  counts[0] = cand.size(); counts[1] = c2[0]; counts[2] = c2[1];
  return kept;
}

extern "C" {

// 0: drf_transform_map accepts T16; 1: it does not
int mt_pose_fault(const float *T16) { return dr::transform_pose_fault(T16) ? 1 : 0; }
// the candidate keys to out (at most cap of them are stored); *in_range = 0 if a candidate fell outside the key range; returns
// their number
size_t mt_plan(const unsigned long long *keys, size_t n, const float *T16, float vs, unsigned long long *out, size_t cap, int *in_range) {
  bool ok = true;
  const std::vector<unsigned long long> c = dr::plan_transform(std::vector<unsigned long long>(keys, keys + n), dr::map_motion(T16, vs), &ok);
  std::copy(c.begin(), c.begin() + (long)std::min(c.size(), cap), out);
  *in_range = ok ? 1 : 0;
  return c.size();
}
// transform_blocks; at most cap blocks are stored to out_keys / out_vox; returns the number of blocks written
size_t mt_transform_blocks(const unsigned long long *keys, const unsigned char *vox, size_t n, const float *T16, float vs, unsigned long long *out_keys,
                           unsigned char *out_vox, size_t cap, unsigned long long counts[3]) {
  std::vector<uint8_t> ov;
  uint64_t c[3];
  const std::vector<unsigned long long> kept = transform_blocks(std::vector<unsigned long long>(keys, keys + n), vox, dr::map_motion(T16, vs), ov, c);
  const size_t m = std::min(kept.size(), cap);
  std::copy(kept.begin(), kept.begin() + (long)m, out_keys);
  if (m) memcpy(out_vox, ov.data(), m * 4096);
  counts[0] = c[0]; counts[1] = c[1]; counts[2] = c[2];
  return kept.size();
}

}  // extern "C"
