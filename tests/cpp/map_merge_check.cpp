// C entry points over the merge half of tandem_amd/csrc/fusion_host.h for tests/test_map_merge.py (plain g++, no HIP):
// merge_voxel / merge_block (the rule of drf_merge_map) and plan_merge (the file-against-map classification).
#include "../../tandem_amd/csrc/fusion_host.h"

extern "C" {

// n voxel pairs (8 bytes each): a[i] merged with b[i] in place, cases[i] = 1, 2 or 3
void mm_merge_voxels(unsigned char *a, const unsigned char *b, size_t n, int W, unsigned char *cases) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t va[2], vb[2];
    memcpy(va, a + 8 * i, 8); memcpy(vb, b + 8 * i, 8);
    cases[i] = (unsigned char)dr::merge_voxel(va, vb, (unsigned char)W);
    memcpy(a + 8 * i, va, 8);
  }
}
// nblocks blocks of src merged into dst; counts[0] += case 2, counts[1] += case 3
void mm_merge_blocks(unsigned char *dst, const unsigned char *src, size_t nblocks, int W, unsigned long long counts[2]) {
  uint64_t c[2] = {counts[0], counts[1]};
  for (size_t i = 0; i < nblocks; ++i) dr::merge_block(dst + i * 4096, src + i * 4096, (unsigned char)W, c);
  counts[0] = c[0]; counts[1] = c[1];
}
// plan_merge flattened: every output array holds nfile entries (bounds: nfile + 2); counts[3] = resident, added, stored; returns
// the number of chunks
size_t mm_plan(const unsigned long long *res, const int *res_slot, size_t nres, const unsigned long long *sto, size_t nsto, const unsigned long long *file,
               size_t nfile, size_t chunk, int *r_src, int *r_slot, int *a_src, unsigned long long *a_key, int *s_src, unsigned long long *s_key,
               unsigned long long *rb, unsigned long long *ab, unsigned long long *sb, unsigned long long counts[3]) {
  const std::vector<unsigned long long> vr(res, res + nres), vs(sto, sto + nsto), vf(file, file + nfile);
  const std::vector<int> slots(res_slot, res_slot + nres);
  const dr::MergePlan p = dr::plan_merge(vr, slots, vs, vf, chunk);
  std::copy(p.res_src.begin(), p.res_src.end(), r_src); std::copy(p.res_slot.begin(), p.res_slot.end(), r_slot);
  std::copy(p.add_src.begin(), p.add_src.end(), a_src); std::copy(p.add_key.begin(), p.add_key.end(), a_key);
  std::copy(p.sto_src.begin(), p.sto_src.end(), s_src); std::copy(p.sto_key.begin(), p.sto_key.end(), s_key);
  std::copy(p.rb.begin(), p.rb.end(), rb); std::copy(p.ab.begin(), p.ab.end(), ab); std::copy(p.sb.begin(), p.sb.end(), sb);
  counts[0] = p.res_src.size(); counts[1] = p.add_src.size(); counts[2] = p.sto_src.size();
  return p.chunks();
}

}  // extern "C"
