// stream_kernels.h -- moving voxel blocks between the device pool and the host store (DESIGN.md "Streaming voxel blocks").
// Included by dr_fusion.hip inside namespace dr, after volume_kernels.h (FusionDev, the block-index helpers) and raycast_kernels.h.
// The host side of streaming is stream_ops.h (BlockStreamer): it alone launches the k_ev_* chain.
//
// Eviction is one chain on the integration stream, launched after the scan's k_fold_counter:
//   k_ev_select    one lane per pool block: blocks whose centre lies beyond the radius (or whose origin lies in a box) go to
//                  the selection list, at most `cap` of them (the rest wait for the next chain)
//   k_ev_gather    one wave per selected block: its key and 4 KB straight into mapped pinned host staging; grid cell and
//                  presence bit cleared, blk_key marked empty
//   k_ev_pair      holes below the new block count <-> surviving blocks of the tail [new n_alloc, old n_alloc)
//   k_ev_move      one wave per pair: a surviving tail block moves into a hole (voxels, key, grid cell)
//   k_ev_zero_tail the vacated tail slots get zero voxels again (k_alloc_commit hands slots out assuming so)
//   k_ev_clear     superblock flags -- and the open-addressing table when it holds blocks -- emptied
//   k_ev_reindex   rebuilt from the surviving blocks [0, new n_alloc)
//   k_ev_finish    n_alloc (and the table's block count) updated, the counts published to pinned memory
// Every kernel after k_ev_select exits at once when the selection is empty.  Stream-in (k_in_place + k_in_finish) appends
// blocks from a pinned upload to the pool and publishes them the way k_alloc_commit does.  The map file (drf_save_map /
// drf_load_map) uses the same two moves: k_map_gather copies pool blocks into a chunk of the file without touching the map,
// and a load places the file's chunks with k_in_place + k_in_finish.  A merge (drf_merge_map) combines the file's blocks whose
// key is resident into their pool slots (k_map_merge) and appends those the map lacks (k_in_place_at + k_in_finish).  A rigid
// resample (drf_transform_map) does not touch the map at all: k_map_transform reads a source map uploaded for the call and writes
// blocks of the destination lattice into a chunk of the output file.  The host side of the four map-file moves: save / load / merge
// are FusionEngine's (dr_fusion.hip), the resample is map_ops.h map_transform; all of them go through MapIo's two chunk pumps.

struct StreamDev {
  int *ctl;                    // [0] blocks selected (uncapped), [1] holes, [2] tail survivors, [3] table blocks re-inserted,
                               // [4] largest squared centre distance of an UNselected block (radius mode; fp32 bits)
  int *list;                   // [cap] pool indices of the selected blocks
  int *mv_dst, *mv_src;        // [cap] compaction pairs
  unsigned long long *h_keys;  // mapped pinned staging (device addresses): keys of the gathered blocks
  uint4 *h_vox;                //   and their voxels, 4 KB per block
  int *h_out;                  // mapped pinned: [0] blocks gathered, [1] blocks selected (uncapped), [2] n_alloc afterwards, [3] = ctl[4]
  int cap;                     // blocks this chain may take (staging size, bounded by the host store's free capacity)
};

__device__ inline int pool_count(const FusionDev &d) { return min(*d.n_alloc, d.o.num_blocks); }
__device__ inline int ev_taken(const StreamDev &s) { return min(s.ctl[0], s.cap); }

// Streaming centre of block P: the centre of the cube of points that map into it, ((8 P + 3.5) voxel_size) per axis
// (voxel g covers ((g - 0.5) vs, (g + 0.5) vs)).  Origin: 8 P voxel_size, the corner k_cull and k_integrate use.
__device__ inline float blk_centre(int c, float vs) { return ((float)(c * kBS) + 3.5f) * vs; }
__device__ inline float blk_origin(int c, float vs) { return (float)(c * kBS) * vs; }

// box == 0: select blocks whose centre lies farther than sqrt(r2) from p;  box != 0: blocks whose origin lies in [lo, hi]
__global__ __launch_bounds__(256) void k_ev_select(const FusionDev d, const StreamDev s, F3 p, float r2, F3 lo, F3 hi, int box) {
  const int n = pool_count(d);
  const float vs = d.o.voxel_size;
  const int lane = threadIdx.x & 63;
  float kept = 0.0f;  // largest squared distance among the blocks that stay (lets the host skip later passes)
  for (int e0 = (blockIdx.x * blockDim.x + threadIdx.x) & ~63; e0 < n; e0 += gridDim.x * blockDim.x) {
    const int e = e0 + lane;
    bool sel = false;
    if (e < n) {
      const I3 P = unpack_key(d.blk_key[e]);
      if (box) {
        const float ox = blk_origin(P.x, vs), oy = blk_origin(P.y, vs), oz = blk_origin(P.z, vs);
        sel = ox >= lo.x && ox <= hi.x && oy >= lo.y && oy <= hi.y && oz >= lo.z && oz <= hi.z;
      } else {
        const float dx = blk_centre(P.x, vs) - p.x, dy = blk_centre(P.y, vs) - p.y, dz = blk_centre(P.z, vs) - p.z;
        const float q = dx * dx + dy * dy + dz * dz;
        sel = q > r2;
        if (!sel) kept = fmaxf(kept, q);
      }
    }
    const unsigned long long m = __ballot(sel);
    if (!m) continue;
    const int leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(&s.ctl[0], __popcll(m));
    base = __builtin_amdgcn_readlane(base, leader);
    if (sel) {
      const int slot = base + __popcll(m & ((1ull << lane) - 1));
      if (slot < s.cap) s.list[slot] = e;
    }
  }
  for (int off = 32; off > 0; off >>= 1) kept = fmaxf(kept, __shfl_xor(kept, off));
  if (lane == 0 && kept > 0.0f) atomicMax(reinterpret_cast<unsigned *>(&s.ctl[4]), __float_as_uint(kept));  // non-negative floats order as their bits
}

__global__ __launch_bounds__(256) void k_ev_gather(const FusionDev d, const StreamDev s) {
  const int m = ev_taken(s);
  if (m == 0) return;
  const int lane = threadIdx.x & 63;
  for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < m; i += gridDim.x * 4) {
    const int e = s.list[i];
    const uint4 *src = reinterpret_cast<const uint4 *>(d.vox + (size_t)e * 512);
    uint4 *dst = s.h_vox + (size_t)i * 256;
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[lane + 64 * k] = src[lane + 64 * k];
    if (lane == 0) {
      const unsigned long long key = d.blk_key[e];
      s.h_keys[i] = key;
      d.blk_key[e] = kEmptyKey;  // k_ev_pair: this slot is not a survivor
      unsigned idx;
      if (grid_index(unpack_key(key), idx)) {
        d.grid[idx] = 0;
        atomicAnd(&d.present[idx >> 5], ~(1u << (idx & 31)));
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_ev_pair(const FusionDev d, const StreamDev s) {
  const int m = ev_taken(s);
  if (m == 0) return;
  const int n2 = pool_count(d) - m;
  // holes = selected blocks below n2; survivors = unselected blocks of [n2, n2 + m): equally many
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
    const int e = s.list[i];
    if (e < n2) s.mv_dst[atomicAdd(&s.ctl[1], 1)] = e;
    if (d.blk_key[n2 + i] != kEmptyKey) s.mv_src[atomicAdd(&s.ctl[2], 1)] = n2 + i;
  }
}

__global__ __launch_bounds__(256) void k_ev_move(const FusionDev d, const StreamDev s) {
  const int nm = s.ctl[1];
  if (nm == 0) return;
  const int lane = threadIdx.x & 63;
  for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < nm; i += gridDim.x * 4) {
    const int src = s.mv_src[i], dst = s.mv_dst[i];
    const uint4 *a = reinterpret_cast<const uint4 *>(d.vox + (size_t)src * 512);
    uint4 *b = reinterpret_cast<uint4 *>(d.vox + (size_t)dst * 512);
#pragma unroll
    for (int k = 0; k < 4; ++k) b[lane + 64 * k] = a[lane + 64 * k];
    if (lane == 0) {
      const unsigned long long key = d.blk_key[src];
      d.blk_key[dst] = key;
      unsigned idx;
      if (grid_index(unpack_key(key), idx)) d.grid[idx] = dst + 1;  // table blocks: k_ev_reindex
    }
  }
}

__global__ __launch_bounds__(256) void k_ev_zero_tail(const FusionDev d, const StreamDev s) {
  const int m = ev_taken(s);
  if (m == 0) return;
  const int n2 = pool_count(d) - m;
  const int lane = threadIdx.x & 63;
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < m; i += gridDim.x * 4) {
    uint4 *b = reinterpret_cast<uint4 *>(d.vox + (size_t)(n2 + i) * 512);
#pragma unroll
    for (int k = 0; k < 4; ++k) b[lane + 64 * k] = z;
  }
}

__global__ __launch_bounds__(256) void k_ev_clear(const FusionDev d, const StreamDev s, unsigned table_cap) {
  if (ev_taken(s) == 0) return;
  const bool table = d.n_alloc[3] != 0;
  const unsigned n0 = 1u << (3 * (kGridBits - kSuperShift[0])), n1 = 1u << (3 * (kGridBits - kSuperShift[1]));
  const unsigned n = max(max(n0, n1), table ? table_cap : 0u);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (i < n0) d.super[0][i] = 0;
    if (i < n1) d.super[1][i] = 0;
    if (table && i < table_cap) { d.keys[i] = kEmptyKey; d.vals[i] = -1; }
  }
}

// insert a block that is known to be absent from the table with its pool index (HashTable::AllocateBlock without the pool)
__device__ inline void table_insert(const FusionDev &d, unsigned long long key, int val) {
  unsigned s = hash_key(key) & d.cmask;
  for (unsigned probe = 0; probe <= d.cmask; ++probe) {
    const unsigned long long cur = atomicCAS(&d.keys[s], kEmptyKey, key);
    if (cur == kEmptyKey || cur == key) {
      __hip_atomic_store(&d.vals[s], val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
    s = (s + 1) & d.cmask;
  }
  d.err[0] = 1;
}

__device__ inline void set_super(const FusionDev &d, unsigned idx) {
  d.super[0][super_index<kSuperShift[0]>(idx)] = 1;
  d.super[1][super_index<kSuperShift[1]>(idx)] = 1;
}

__global__ __launch_bounds__(256) void k_ev_reindex(const FusionDev d, const StreamDev s) {
  const int m = ev_taken(s);
  if (m == 0) return;
  const bool table = d.n_alloc[3] != 0;
  const int n2 = pool_count(d) - m;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n2; e += gridDim.x * blockDim.x) {
    const unsigned long long key = d.blk_key[e];
    unsigned idx;
    if (grid_index(unpack_key(key), idx)) set_super(d, idx);
    else if (table) { table_insert(d, key, e); atomicAdd(&s.ctl[3], 1); }
  }
}

__global__ void k_ev_finish(const FusionDev d, const StreamDev s) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int raw = s.ctl[0], m = min(raw, s.cap);
  int n = pool_count(d);
  if (m > 0) {
    n -= m;
    d.n_alloc[0] = n;
    if (d.n_alloc[3] != 0) d.n_alloc[3] = s.ctl[3];
  }
  s.h_out[0] = m; s.h_out[1] = raw; s.h_out[2] = n; s.h_out[3] = s.ctl[4];
  s.ctl[0] = s.ctl[1] = s.ctl[2] = s.ctl[3] = s.ctl[4] = 0;
}

// Stream-in: n blocks from the pinned upload (keys, 4 KB each) appended at the end of the pool.  The host has checked that
// they fit and that none of them is resident.
__global__ __launch_bounds__(256) void k_in_place(const FusionDev d, const unsigned long long *__restrict__ keys, const uint4 *__restrict__ vox, int n) {
  const int base = pool_count(d);
  const int lane = threadIdx.x & 63;
  for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {
    const int p = base + i;
    const uint4 *a = vox + (size_t)i * 256;
    uint4 *b = reinterpret_cast<uint4 *>(d.vox + (size_t)p * 512);
#pragma unroll
    for (int k = 0; k < 4; ++k) b[lane + 64 * k] = a[lane + 64 * k];
    if (lane == 0) {
      const unsigned long long key = keys[i];
      d.blk_key[p] = key;
      unsigned idx;
      if (grid_index(unpack_key(key), idx)) {
        d.grid[idx] = p + 1;
        atomicOr(&d.present[idx >> 5], 1u << (idx & 31));
        set_super(d, idx);
      } else {
        table_insert(d, key, p);
        atomicAdd(&d.n_alloc[3], 1);
      }
    }
  }
}
__global__ void k_in_finish(int *n_alloc, int n) {
  if (threadIdx.x == 0 && blockIdx.x == 0) n_alloc[0] += n;
}

// Map save: pool block src[i] -> position dst[i] of the chunk buffer `out` (mapped pinned memory the file is written from),
// i in [0, n): one wave per block, four uint4 per lane.  Writes nothing else -- grid, presence bits and blk_key stay as they are.
__global__ __launch_bounds__(256) void k_map_gather(const Voxel *__restrict__ vox, const int *__restrict__ src, const int *__restrict__ dst, int n,
                                                    uint4 *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {
    const uint4 *a = reinterpret_cast<const uint4 *>(vox + (size_t)src[i] * 512);
    uint4 *b = out + (size_t)dst[i] * 256;
#pragma unroll
    for (int k = 0; k < 4; ++k) b[lane + 64 * k] = a[lane + 64 * k];
  }
}

// Map merge: block src[i] of the chunk buffer (mapped pinned memory, read once) combined into pool slot slot[i], i in [0, n):
// one wave per block, four uint4 = 8 voxels per lane, merge_voxel (fusion_host.h: the rule) on each.  A voxel of case 1 is
// written back with the bytes it was read with.  counts[0] += voxels of case 2, counts[1] += voxels of case 3: summed across
// the wave, one atomic each per wave.  Touches nothing but the voxels: keys, grid, presence bits stay as they are.
__global__ __launch_bounds__(256) void k_map_merge(Voxel *__restrict__ vox, const int *__restrict__ src, const int *__restrict__ slot, int n,
                                                   const uint4 *__restrict__ chunk, unsigned char W, unsigned long long *__restrict__ counts) {
  const int lane = threadIdx.x & 63;
  unsigned n2 = 0, n3 = 0;
  for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {
    const uint4 *b = chunk + (size_t)src[i] * 256;
    uint4 *a = reinterpret_cast<uint4 *>(vox + (size_t)slot[i] * 512);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint4 vb = b[lane + 64 * k];
      uint4 va = a[lane + 64 * k];
      uint32_t p[2] = {va.x, va.y}, q[2] = {va.z, va.w};
      const uint32_t pb[2] = {vb.x, vb.y}, qb[2] = {vb.z, vb.w};
      const int c0 = merge_voxel(p, pb, W), c1 = merge_voxel(q, qb, W);
      n2 += (c0 == 2) + (c1 == 2);
      n3 += (c0 == 3) + (c1 == 3);
      a[lane + 64 * k] = make_uint4(p[0], p[1], q[0], q[1]);
    }
  }
  for (int off = 32; off > 0; off >>= 1) { n2 += __shfl_xor(n2, off); n3 += __shfl_xor(n3, off); }
  if (lane == 0) {
    if (n2) atomicAdd(&counts[0], (unsigned long long)n2);
    if (n3) atomicAdd(&counts[1], (unsigned long long)n3);
  }
}

// k_in_place with a source index list: key keys[i] and block src[i] of the chunk buffer -> pool slot n_alloc + i.  A chunk's
// added blocks are not contiguous in its buffer.  Followed by k_in_finish like k_in_place.
__global__ __launch_bounds__(256) void k_in_place_at(const FusionDev d, const unsigned long long *__restrict__ keys, const int *__restrict__ src,
                                                     const uint4 *__restrict__ vox, int n) {
  const int base = pool_count(d);
  const int lane = threadIdx.x & 63;
  for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {
    const int p = base + i;
    const uint4 *a = vox + (size_t)src[i] * 256;
    uint4 *b = reinterpret_cast<uint4 *>(d.vox + (size_t)p * 512);
#pragma unroll
    for (int k = 0; k < 4; ++k) b[lane + 64 * k] = a[lane + 64 * k];
    if (lane == 0) {
      const unsigned long long key = keys[i];
      d.blk_key[p] = key;
      unsigned idx;
      if (grid_index(unpack_key(key), idx)) {
        d.grid[idx] = p + 1;
        atomicOr(&d.present[idx >> 5], 1u << (idx & 31));
        set_super(d, idx);
      } else {
        table_insert(d, key, p);
        atomicAdd(&d.n_alloc[3], 1);
      }
    }
  }
}

// ---- drf_transform_map: a map file resampled on the lattice of another world frame (the rule: fusion_host.h transform_voxel)
// slot of block (bx, by, bz) in the ascending key table keys[0, n), or -1 (absent, or outside the key range)
__device__ __forceinline__ int xf_find(const unsigned long long *__restrict__ keys, int n, int bx, int by, int bz) {
  const int B = 1 << 20;
  if (bx < -B || bx >= B || by < -B || by >= B || bz < -B || bz >= B) return -1;
  const unsigned long long key = ((unsigned long long)(bx + B) << 42) | ((unsigned long long)(by + B) << 21) | (unsigned long long)(bz + B);
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return (lo < n && keys[lo] == key) ? lo : -1;
}
// transform_voxel's fetch on the device: the 3^3 source blocks from block nb0 on were resolved once per wave (near[27], LDS);
// a corner outside them -- which the extent argument below rules out up to rounding -- searches the table itself
struct XfFetch {
  const unsigned long long *keys;
  const uint2 *vox;
  const int *near;
  int n, nb0[3];
  __device__ __forceinline__ void operator()(int x, int y, int z, uint32_t v[2]) const {
    const int bx = x >> 3, by = y >> 3, bz = z >> 3;
    const unsigned rx = (unsigned)(bx - nb0[0]), ry = (unsigned)(by - nb0[1]), rz = (unsigned)(bz - nb0[2]);
    const int slot = (rx < 3u && ry < 3u && rz < 3u) ? near[rx * 9 + ry * 3 + rz] : xf_find(keys, n, bx, by, bz);
    if (slot < 0) { v[0] = 0; v[1] = 0; return; }
    const uint2 q = vox[(size_t)slot * 512 + (size_t)(((x & 7) << 6) | ((y & 7) << 3) | (z & 7))];
    v[0] = q.x; v[1] = q.y;
  }
};
// One wave per destination block dst_keys[i], i in [0, nd) (no grid stride: the workgroup's four waves meet at one barrier), four
// uint4 = 8 voxels per lane.  The image of a destination block under u = R^T (g - tv) is a rotated 7-voxel cube, at most
// 7 sqrt(3) + 1 voxels along an axis with its trilinear corners: it spans at most 3 source blocks per axis.  So 27 lanes first
// resolve the blocks from nb0 = floor(min over the block's 8 corner voxels of floor(u) / 8) on, one binary search each in the
// source's ascending key table, into LDS, and the 8 corner reads per voxel look blocks up there.
// kWrite = false, the count pass: flags[i] = the block holds a weighted voxel, counts[0] += voxels with weight > 0,
// counts[1] += voxels refused (summed across the wave, one atomic each per wave).  kWrite = true, the write pass over the blocks
// the count pass kept: block i to out + i * 256 (a chunk of the file in mapped pinned memory, written once).
template <bool kWrite>
__global__ __launch_bounds__(256) void k_map_transform(const unsigned long long *__restrict__ src_keys, const uint2 *__restrict__ src_vox, int n,
                                                       const unsigned long long *__restrict__ dst_keys, int nd, const MapMotion m,
                                                       uint4 *__restrict__ out, int *__restrict__ flags, unsigned long long *__restrict__ counts) {
  __shared__ int s_near[4][27];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave;
  const bool live = i < nd;
  int blk[3] = {0, 0, 0};
  XfFetch fetch;
  fetch.keys = src_keys; fetch.vox = src_vox; fetch.near = s_near[wave]; fetch.n = n;
  fetch.nb0[0] = fetch.nb0[1] = fetch.nb0[2] = 0;
  if (live) {
    const unsigned long long key = dst_keys[i];
    blk[0] = (int)((key >> 42) & 0x1fffff) - (1 << 20);
    blk[1] = (int)((key >> 21) & 0x1fffff) - (1 << 20);
    blk[2] = (int)(key & 0x1fffff) - (1 << 20);
    double lo[3] = {1073741824.0, 1073741824.0, 1073741824.0};
    for (int e = 0; e < 8; ++e) {
      const double d0 = (double)(blk[0] * 8 + ((e & 4) ? 7 : 0)) - m.tv[0], d1 = (double)(blk[1] * 8 + ((e & 2) ? 7 : 0)) - m.tv[1],
                   d2 = (double)(blk[2] * 8 + ((e & 1) ? 7 : 0)) - m.tv[2];
      for (int k = 0; k < 3; ++k) {
        const double u = (m.R[k] * d0 + m.R[3 + k] * d1) + m.R[6 + k] * d2;
        lo[k] = u < lo[k] ? u : lo[k];
      }
    }
    for (int k = 0; k < 3; ++k) {
      const double c = lo[k] > -1073741824.0 ? lo[k] : -1073741824.0;  // (beyond it transform_voxel reads nothing)
      fetch.nb0[k] = (int)floor(c) >> 3;
    }
    if (lane < 27) s_near[wave][lane] = xf_find(src_keys, n, fetch.nb0[0] + lane / 9, fetch.nb0[1] + (lane / 3) % 3, fetch.nb0[2] + lane % 3);
  }
  __syncthreads();
  unsigned nw = 0, nr = 0;
  if (live) {
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
      const int v = 2 * (lane + 64 * k);  // voxels v and v + 1: neighbours along z
      const int gx = blk[0] * 8 + (v >> 6), gy = blk[1] * 8 + ((v >> 3) & 7), gz = blk[2] * 8 + (v & 7);
      uint32_t p[2], q[2];
      const int c0 = transform_voxel(m, gx, gy, gz, fetch, p), c1 = transform_voxel(m, gx, gy, gz + 1, fetch, q);
      nw += (c0 == 1) + (c1 == 1);
      nr += (c0 == 2) + (c1 == 2);
      if (kWrite) out[(size_t)i * 256 + lane + 64 * k] = make_uint4(p[0], p[1], q[0], q[1]);
    }
  }
  if (!kWrite) {
    for (int off = 32; off > 0; off >>= 1) { nw += __shfl_xor(nw, off); nr += __shfl_xor(nr, off); }
    if (live && lane == 0) {
      flags[i] = nw > 0;
      if (nw) atomicAdd(&counts[0], (unsigned long long)nw);
      if (nr) atomicAdd(&counts[1], (unsigned long long)nr);
    }
  }
}
