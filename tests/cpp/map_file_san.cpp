// Stand-alone run of tandem_amd/csrc/map_file.h for a sanitizer build (tests/test_map_file.py builds it with
// g++ -fsanitize=address,undefined and runs it): seeded writes, reads with several chunk sizes, and every refusal.
//   map_file_san DIR      exits 0 when every check holds
#include <random>

#include "../../tandem_amd/csrc/map_file.h"

static int g_bad = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "map_file_san: line %d: %s\n", __LINE__, #c); ++g_bad; } } while (0)

static std::vector<unsigned char> slurp(const std::string &p) {
  std::vector<unsigned char> v;
  FILE *f = fopen(p.c_str(), "rb");
  if (!f) return v;
  unsigned char buf[65536];
  for (size_t m; (m = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + m);
  fclose(f);
  return v;
}
static void spit(const std::string &p, const std::vector<unsigned char> &v, size_t bytes) {
  FILE *f = fopen(p.c_str(), "wb");
  if (!f) { ++g_bad; return; }
  if (bytes && fwrite(v.data(), 1, bytes, f) != bytes) ++g_bad;
  fclose(f);
}
static bool exists(const std::string &p) {
  FILE *f = fopen(p.c_str(), "rb");
  if (f) fclose(f);
  return f != nullptr;
}
static bool refused(const std::string &p) {
  std::string err;
  float vs;
  uint64_t n;
  const bool ok = dr::map_file_info(p, &vs, &n, err);
  return !ok && !err.empty();
}

static void round_trip(const std::string &dir, uint64_t n, unsigned seed) {
  std::mt19937_64 rng(seed);
  const long B = dr::kKeyBias;
  std::vector<unsigned long long> keys;
  if (n > 0) keys.push_back(dr::pack_biased(-B + 1, -B + 1, -B + 1));
  if (n > 1) keys.push_back(dr::pack_biased(B - 1, B - 1, B - 1));
  while (keys.size() < n) keys.push_back(dr::pack_biased((long)(rng() % 600) - 300, (long)(rng() % 600) - 300, (long)(rng() % 600) - 300));
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  n = keys.size();
  std::vector<unsigned char> vox((size_t)n * 4096 + 1);
  for (auto &b : vox) b = (unsigned char)rng();
  const std::string path = dir + "/m" + std::to_string(n) + ".drfmap";
  const float vs = 0.02f;
  std::string err;
  for (size_t wchunk : {(size_t)0, (size_t)1, (size_t)7}) {
    dr::MapWriter w;
    CHECK(w.open(path, vs, keys.data(), n, err));
    CHECK(exists(path + ".part"));
    const size_t step = wchunk ? wchunk : (size_t)std::max<uint64_t>(n, 1);
    for (uint64_t b = 0; b < n; b += step) CHECK(w.append(vox.data() + b * 4096, (size_t)std::min<uint64_t>(step, n - b), err));
    CHECK(w.close(err));
    CHECK(!exists(path + ".part") && exists(path));
    CHECK(slurp(path).size() == 72 + 4104 * n);
  }
  for (size_t rchunk : {(size_t)1, (size_t)7, (size_t)64, (size_t)0}) {
    dr::MapReader r;
    CHECK(r.open(path, err));
    CHECK(r.blocks() == n && r.voxel_size() == vs && r.keys() == keys);
    std::vector<unsigned char> back((size_t)n * 4096 + 1);
    const size_t step = rchunk ? rchunk : (size_t)std::max<uint64_t>(n, 1);
    while (r.remaining()) {
      const uint64_t at = n - r.remaining();
      CHECK(r.read(back.data() + at * 4096, (size_t)std::min<uint64_t>(step, r.remaining()), err));
    }
    CHECK(!r.read(back.data(), 1, err));
    CHECK(r.verified());
    CHECK(memcmp(back.data(), vox.data(), (size_t)n * 4096) == 0);
  }
  // refusals: each variant of the good file is refused
  const std::vector<unsigned char> good = slurp(path);
  const std::string bad = dir + "/bad.drfmap";
  auto variant = [&](size_t at, unsigned char x) {
    std::vector<unsigned char> v = good;
    v[at] ^= x;
    spit(bad, v, v.size());
    CHECK(refused(bad));
  };
  variant(0, 1);    // magic
  variant(8, 1);    // header size
  variant(12, 1);   // block edge
  variant(16, 16);  // voxel bytes
  variant(24, 1);   // n: the size no longer matches
  variant(40, 1);   // a reserved byte
  variant(good.size() - 1, 0x80);  // the checksum
  for (size_t cut : {(size_t)0, (size_t)10, (size_t)63, (size_t)71, good.size() - 1}) {
    spit(bad, good, std::min(cut, good.size()));
    CHECK(refused(bad));
  }
  {
    std::vector<unsigned char> v = good;
    v.push_back(0);
    spit(bad, v, v.size());
    CHECK(refused(bad));
  }
  if (n > 0) {
    variant(64 + 8 * n + 17, 4);  // a voxel bit
    spit(bad, good, 64 + 8 * (size_t)n - 3);  // cut in the key table
    CHECK(refused(bad));
    spit(bad, good, 64 + 8 * (size_t)n + 4096 / 2);  // in the payload
    CHECK(refused(bad));
  }
  if (n > 1) {
    std::vector<unsigned char> v = good;  // two equal keys / a descending pair: the checksum made right again, the order alone refuses
    for (int mode = 0; mode < 2; ++mode) {
      v = good;
      if (mode == 0) memcpy(&v[64 + 8], &v[64], 8);
      else for (int k = 0; k < 8; ++k) std::swap(v[64 + k], v[64 + 8 + k]);
      const uint64_t h = dr::map_hash(dr::kMapHashSeed, v.data() + 64, v.size() - 72);
      memcpy(&v[v.size() - 8], &h, 8);
      spit(bad, v, v.size());
      CHECK(refused(bad));
    }
    dr::MapWriter w;  // and the writer refuses them too, leaving nothing behind
    std::vector<unsigned long long> k2 = keys;
    k2[1] = k2[0];
    CHECK(!w.open(bad + "2", vs, k2.data(), n, err) && !exists(bad + "2.part"));
  }
  {
    dr::MapWriter w;  // a directory that does not exist
    CHECK(!w.open(dir + "/no/such/dir/m.drfmap", vs, keys.data(), n, err));
    CHECK(!exists(dir + "/no/such/dir/m.drfmap") && !exists(dir + "/no/such/dir/m.drfmap.part"));
  }
  {
    dr::MapWriter w;  // abandoned half way: the .part goes, the earlier good file stays
    CHECK(w.open(path, vs, keys.data(), n, err));
    if (n > 0) CHECK(w.append(vox.data(), 1, err));
    if (n > 1) { CHECK(!w.close(err)); }  // fewer blocks than keys
    else w.abandon();
    CHECK(!exists(path + ".part") && slurp(path) == good);
  }
  CHECK(!refused(path));
  if (n >= 3) {  // the file changes between open() and the reads: every read() succeeds, verify() says so; unchanged, it holds
    for (int change = 0; change < 2; ++change) {
      dr::MapReader r;
      CHECK(r.open(path, err));
      if (change) {  // one byte in the middle of the last block, through a second handle
        const size_t at = 64 + 8 * (size_t)n + 4096 * ((size_t)n - 1) + 2048;
        FILE *f = fopen(path.c_str(), "r+b");
        CHECK(f && fseek(f, (long)at, SEEK_SET) == 0 && fputc(good[at] ^ 0x20, f) != EOF);
        if (f) CHECK(fclose(f) == 0);
      }
      std::vector<unsigned char> block(4096);
      while (r.remaining()) CHECK(r.read(block.data(), 1, err));
      err.clear();
      CHECK(r.verify(err) == !change && r.verified() == !change);
      CHECK(err == (change ? "map file " + path + " changed while it was read" : std::string()));
    }
    CHECK(refused(path));
  }
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: map_file_san DIR\n"); return 2; }
  for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)300}) round_trip(argv[1], n, 17 + (unsigned)n);
  if (g_bad) { fprintf(stderr, "map_file_san: %d checks failed\n", g_bad); return 1; }
  printf("map_file_san ok\n");
  return 0;
}
