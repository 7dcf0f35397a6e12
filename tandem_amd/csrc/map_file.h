// map_file.h -- the DrFusion map file (include/dr_mi355x.h "map files"): a streaming writer and a validating reader.  Plain
// C++17, no HIP header, depends on fusion_host.h only, so all of it runs in the CPU tests (tests/cpp/map_file_check.cpp).
// Nothing here throws on a file failure: every call returns false and says why in `err`; the engine (dr_fusion.hip) turns
// that into DR_ERR_IO.
//
// Layout, little-endian, 72 + 4104 n bytes:
//   0   8 bytes "DRFMAP01"        8  u32 header size = 64      12  u32 block edge = 8      16  u32 bytes per voxel = 8
//   20  f32 voxel_size (bits)     24 u64 n = blocks            32  32 reserved bytes, zero
//   64            n x u64 packed block keys (pack_biased), strictly ascending
//   64 + 8 n      n x 4096 bytes of voxels in the keys' order ({f32 sdf, u8 b, g, r, u8 weight}, index x*64 + y*8 + z)
//   64 + 4104 n   u64 checksum over key table and voxels: h = 0xcbf29ce484222325; per u64 word w: h = (h ^ w) * 0x100000001b3
#pragma once
#include <cstdio>
#include <string>

#include "fusion_host.h"

namespace dr {

#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ != __ORDER_LITTLE_ENDIAN__
#error "map_file.h writes host words as they lie in memory: little-endian hosts only"
#endif

constexpr char kMapMagic[8] = {'D', 'R', 'F', 'M', 'A', 'P', '0', '1'};
constexpr uint32_t kMapHeaderBytes = 64, kMapVoxelBytes = 8;
constexpr size_t kMapBlockBytes = 4096;  // kBS^3 voxels
constexpr uint64_t kMapHashSeed = 0xcbf29ce484222325ull, kMapHashPrime = 0x100000001b3ull;
constexpr uint64_t kMapMaxBlocks = ((uint64_t)1 << 62) / 4104;  // far beyond any file; keeps 72 + 4104 n in 63 bits

// the checksum continued over `bytes` bytes (a multiple of 8) at p
inline uint64_t map_hash(uint64_t h, const void *p, size_t bytes) {
  const unsigned char *b = (const unsigned char *)p;
  for (size_t i = 0; i + 8 <= bytes; i += 8) {
    uint64_t w;
    memcpy(&w, b + i, 8);
    h = (h ^ w) * kMapHashPrime;
  }
  return h;
}
// strictly ascending and below 2^63
inline bool map_keys_ok(const unsigned long long *keys, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i)
    if ((keys[i] >> 63) || (i && keys[i] <= keys[i - 1])) return false;
  return true;
}

// Header, key table, then the blocks appended in the keys' order, then the trailer.  Everything goes to <path>.part, which
// becomes <path> when close() succeeds; any failure, or a writer that goes away unfinished, removes it.
class MapWriter {
 public:
  MapWriter() = default;
  MapWriter(const MapWriter &) = delete;
  void operator=(const MapWriter &) = delete;
  ~MapWriter() { abandon(); }
  bool open(const std::string &path, float voxel_size, const unsigned long long *keys, uint64_t n, std::string &err) {
    abandon();
    if (!map_keys_ok(keys, n) || n > kMapMaxBlocks) { err = "map file " + path + ": block keys are not strictly ascending"; return false; }
    path_ = path; part_ = path + ".part";
    f_ = fopen(part_.c_str(), "wb");
    if (!f_) { err = "cannot create " + part_; return false; }
    unsigned char head[kMapHeaderBytes] = {0};
    const uint32_t hb = kMapHeaderBytes, edge = (uint32_t)kBS, vb = kMapVoxelBytes;
    memcpy(head, kMapMagic, 8);
    memcpy(head + 8, &hb, 4); memcpy(head + 12, &edge, 4); memcpy(head + 16, &vb, 4);
    memcpy(head + 20, &voxel_size, 4);
    memcpy(head + 24, &n, 8);
    n_ = n; done_ = 0;
    hash_ = map_hash(kMapHashSeed, keys, (size_t)n * 8);
    if (fwrite(head, 1, sizeof head, f_) != sizeof head || (n && fwrite(keys, 8, (size_t)n, f_) != (size_t)n)) return io_fail(err);
    return true;
  }
  // the next `blocks` blocks, 4096 bytes each
  bool append(const void *vox, size_t blocks, std::string &err) {
    if (!f_) { err = "map file " + path_ + ": not open"; return false; }
    if (blocks > n_ - done_) { abandon(); err = "map file " + path_ + ": more blocks than keys"; return false; }
    if (blocks == 0) return true;
    hash_ = map_hash(hash_, vox, blocks * kMapBlockBytes);
    if (fwrite(vox, kMapBlockBytes, blocks, f_) != blocks) return io_fail(err);
    done_ += blocks;
    return true;
  }
  bool close(std::string &err) {
    if (!f_) { err = "map file " + path_ + ": not open"; return false; }
    if (done_ != n_) { abandon(); err = "map file " + path_ + ": fewer blocks than keys"; return false; }
    if (fwrite(&hash_, 8, 1, f_) != 1) return io_fail(err);
    FILE *f = f_;
    f_ = nullptr;
    if (fclose(f) != 0 || rename(part_.c_str(), path_.c_str()) != 0) {
      remove(part_.c_str());
      err = "cannot write " + path_;
      return false;
    }
    return true;
  }
  void abandon() {
    if (!f_) return;
    fclose(f_);
    f_ = nullptr;
    remove(part_.c_str());
  }

 private:
  bool io_fail(std::string &err) {
    abandon();
    err = "write to " + part_ + " failed";
    return false;
  }
  FILE *f_ = nullptr;
  std::string path_, part_;
  uint64_t n_ = 0, done_ = 0, hash_ = 0;
};

// open() validates the WHOLE file -- size against n, magic, header size, block edge, voxel bytes, reserved bytes, keys
// strictly ascending and below 2^63, checksum -- reading it once through a bounded buffer; it never reads beyond the size
// it found.  Then read() hands out the blocks in order, and verified() tells whether that second pass met the same bytes.
class MapReader {
 public:
  MapReader() = default;
  MapReader(const MapReader &) = delete;
  void operator=(const MapReader &) = delete;
  ~MapReader() { if (f_) fclose(f_); }
  bool open(const std::string &path, std::string &err) {
    if (f_) { fclose(f_); f_ = nullptr; }
    path_ = path;
    keys_.clear(); n_ = 0; next_ = 0;
    f_ = fopen(path.c_str(), "rb");
    if (!f_) { err = "cannot open " + path; return false; }
    if (fseek(f_, 0, SEEK_END) != 0) return refuse(err, "cannot be measured");
    const long end = ftell(f_);
    if (end < 0 || fseek(f_, 0, SEEK_SET) != 0) return refuse(err, "cannot be measured");
    const uint64_t size = (uint64_t)end;
    if (size < kMapHeaderBytes + 8) return refuse(err, "is shorter than an empty map file");
    unsigned char head[kMapHeaderBytes];
    if (fread(head, 1, sizeof head, f_) != sizeof head) return refuse(err, "cannot be read");
    uint32_t hb, edge, vb;
    uint64_t n;
    memcpy(&hb, head + 8, 4); memcpy(&edge, head + 12, 4); memcpy(&vb, head + 16, 4); memcpy(&voxel_size_, head + 20, 4); memcpy(&n, head + 24, 8);
    if (memcmp(head, kMapMagic, 8) != 0) return refuse(err, "is not a DrFusion map file (magic)");
    if (hb != kMapHeaderBytes) return refuse(err, "has an unknown header size");
    if (edge != (uint32_t)kBS) return refuse(err, "has a block edge other than 8");
    if (vb != kMapVoxelBytes) return refuse(err, "has a voxel size other than 8 bytes");
    for (size_t i = 32; i < kMapHeaderBytes; ++i)
      if (head[i]) return refuse(err, "has non-zero reserved bytes");
    if (n > kMapMaxBlocks || size != kMapHeaderBytes + 8 + n * (8 + kMapBlockBytes)) return refuse(err, "has a size that does not match its block count");
    keys_.resize((size_t)n);
    if (n && fread(keys_.data(), 8, (size_t)n, f_) != (size_t)n) return refuse(err, "cannot be read");
    if (!map_keys_ok(keys_.data(), n)) return refuse(err, "has block keys that are not strictly ascending");
    uint64_t h = map_hash(kMapHashSeed, keys_.data(), (size_t)n * 8);
    std::vector<unsigned char> buf(std::min<uint64_t>(std::max<uint64_t>(n, 1), 256) * kMapBlockBytes);
    for (uint64_t b = 0; b < n;) {
      const size_t m = (size_t)std::min<uint64_t>(n - b, buf.size() / kMapBlockBytes);
      if (fread(buf.data(), kMapBlockBytes, m, f_) != m) return refuse(err, "cannot be read");
      h = map_hash(h, buf.data(), m * kMapBlockBytes);
      b += m;
    }
    uint64_t want;
    if (fread(&want, 8, 1, f_) != 1) return refuse(err, "cannot be read");
    if (want != h) return refuse(err, "fails its checksum");
    if (fseek(f_, (long)(kMapHeaderBytes + n * 8), SEEK_SET) != 0) return refuse(err, "cannot be read");
    n_ = n; sum_ = want;
    hash_ = map_hash(kMapHashSeed, keys_.data(), (size_t)n * 8);
    return true;
  }
  float voxel_size() const { return voxel_size_; }
  uint64_t blocks() const { return n_; }
  uint64_t checksum() const { return sum_; }
  const std::vector<unsigned long long> &keys() const { return keys_; }
  uint64_t remaining() const { return n_ - next_; }
  // the next `blocks` blocks (at most remaining()) to dst
  bool read(void *dst, size_t blocks, std::string &err) {
    if (!f_ || blocks > n_ - next_) { err = "map file " + path_ + ": read beyond its blocks"; return false; }
    if (blocks == 0) return true;
    if (fread(dst, kMapBlockBytes, blocks, f_) != blocks) { err = "map file " + path_ + " cannot be read"; return false; }
    hash_ = map_hash(hash_, dst, blocks * kMapBlockBytes);
    next_ += blocks;
    return true;
  }
  // every block has been handed out and they were the bytes open() validated
  bool verified() const { return next_ == n_ && hash_ == sum_; }
  // verified(), with the reason in err when it is not
  bool verify(std::string &err) const {
    if (!verified()) err = "map file " + path_ + " changed while it was read";
    return verified();
  }

 private:
  bool refuse(std::string &err, const char *why) {
    err = "map file " + path_ + " " + why;
    if (f_) fclose(f_);
    f_ = nullptr;
    keys_.clear(); n_ = 0;
    return false;
  }
  FILE *f_ = nullptr;
  std::string path_;
  std::vector<unsigned long long> keys_;
  float voxel_size_ = 0.0f;
  uint64_t n_ = 0, next_ = 0, sum_ = 0, hash_ = 0;
};

// the whole file validated; its voxel size and block count
inline bool map_file_info(const std::string &path, float *voxel_size, uint64_t *blocks, std::string &err) {
  MapReader r;
  if (!r.open(path, err)) return false;
  if (voxel_size) *voxel_size = r.voxel_size();
  if (blocks) *blocks = r.blocks();
  return true;
}

}  // namespace dr
