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
// open() validates the file; then -- change != 0 -- a second handle flips one byte in the middle of the LAST block (far from
// anything the validation pass may have left in a stdio buffer); then every block is read, one per read().  0 = every read
// succeeded and verify() held, 5 = every read succeeded and verify() refused (its message in mf_last_error), else what failed.
int mf_read_changed(const char *path, int change) {
  dr::MapReader r;
  if (!r.open(path, g_err)) return 1;
  if (r.blocks() < 3) { g_err = "fewer than 3 blocks"; return 2; }
  if (change) {
    FILE *f = fopen(path, "r+b");
    const long at = (long)(64 + r.blocks() * 8 + (r.blocks() - 1) * 4096 + 2048);
    int c = EOF;
    if (!f || fseek(f, at, SEEK_SET) != 0 || (c = fgetc(f)) == EOF || fseek(f, at, SEEK_SET) != 0 || fputc(c ^ 0x20, f) == EOF || fclose(f) != 0) {
      g_err = "cannot change the file";
      return 2;
    }
  }
  std::vector<unsigned char> block(4096);
  while (r.remaining())
    if (!r.read(block.data(), 1, g_err)) return 3;
  g_err.clear();
  const bool same = r.verify(g_err);
  if (same != r.verified() || same != g_err.empty()) return 4;
  return same ? 0 : 5;
}

}  // extern "C"
