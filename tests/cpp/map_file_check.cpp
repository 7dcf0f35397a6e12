// C entry points over tandem_amd/csrc/map_file.h for tests/test_map_file.py (plain g++, no HIP).
#include "../../tandem_amd/csrc/map_file.h"

static std::string g_err;

extern "C" {

const char *mf_last_error() { return g_err.c_str(); }

// n blocks (keys ascending, 4096 bytes each) through the streaming writer, `chunk` blocks per append (0 = all at once); 0 = written
int mf_write(const char *path, float voxel_size, const unsigned long long *keys, unsigned long long n, const unsigned char *vox, size_t chunk) {
  dr::MapWriter w;
  if (!w.open(path, voxel_size, keys, n, g_err)) return 1;
  if (chunk == 0) chunk = n ? (size_t)n : 1;
  for (unsigned long long b = 0; b < n; b += chunk) {
    const size_t m = (size_t)std::min<unsigned long long>(chunk, n - b);
    if (!w.append(vox + b * 4096, m, g_err)) return 2;
  }
  return w.close(g_err) ? 0 : 3;
}
// a writer that opens and goes away without close(): nothing may stay behind
int mf_write_abandoned(const char *path, float voxel_size, const unsigned long long *keys, unsigned long long n) {
  dr::MapWriter w;
  return w.open(path, voxel_size, keys, n, g_err) ? 0 : 1;
}
int mf_info(const char *path, float *voxel_size, unsigned long long *n) {
  uint64_t blocks = 0;
  if (!dr::map_file_info(path, voxel_size, &blocks, g_err)) return 1;
  *n = blocks;
  return 0;
}
// validates, then reads `chunk` blocks at a time (0 = all at once) into vox (room for cap blocks); 0 = read and verified
int mf_read(const char *path, size_t chunk, float *voxel_size, unsigned long long *n, unsigned long long *keys, unsigned char *vox, unsigned long long cap,
            unsigned long long *checksum) {
  dr::MapReader r;
  if (!r.open(path, g_err)) return 1;
  *voxel_size = r.voxel_size(); *n = r.blocks(); *checksum = r.checksum();
  if (r.blocks() > cap) { g_err = "not enough room"; return 2; }
  if (r.blocks()) memcpy(keys, r.keys().data(), (size_t)r.blocks() * 8);
  if (chunk == 0) chunk = r.blocks() ? (size_t)r.blocks() : 1;
  for (unsigned long long b = 0; b < r.blocks(); b += chunk) {
    const size_t m = (size_t)std::min<unsigned long long>(chunk, r.remaining());
    if (!r.read(vox + b * 4096, m, g_err)) return 3;
  }
  if (r.read(vox, 1, g_err)) return 4;  // beyond the last block: refused
  return r.verified() ? 0 : 5;
}

}  // extern "C"
