// K34 — the cloud thinned on a voxel grid: one centroid record (x, y, z, intensity) per occupied voxel, in the order
// of the voxels' first points.  ops/voxel_downsample.py has the definition; these kernels give its bytes.
//
// Batched over B <= 64 clouds that share one field layout.  Raw PointCloud2 bytes are read in place
// (tca_cloud_load.h).  A dense 3D plane does not fit (160 m x 160 m x 8 m at 0.2 m: 25.6 M cells a cloud), so every
// cloud has an open-addressed hash table in global memory: slots[b] entries (a power of two, at least the cloud's
// points) of 48 bytes, the accumulators in the slot itself:
//
//     key int64 | sum x, y, z, intensity int64 | count int32 | first int32
//
// The key packs the three voxel indices (21 bits each); an empty slot has key -1, which no voxel has.  A slot is
// claimed with one 64-bit compare-and-swap on its key, linear probing, wrapping; whoever finds or claims it adds with
// 64-bit integer atomics and takes an atomicMin of its point index into `first`.  A cloud never has more voxels than
// points, so with slots >= points a probe always ends at the key or at an empty slot, even in a full table.  The
// accumulators live in the slot, not in a dense array behind an id from a counter: an id would have to be published
// by the claiming thread and waited for by every other thread of the voxel, and no workgroup here waits on another.
// The price is the reset, 48 bytes a slot, three 16-byte stores.
//
//   reset    every slot of every table: key -1, sums 0, count 0, first INT32_MAX.
//   insert   blockIdx.y = cloud; a workgroup owns a contiguous span of 2048 points, 256 at a time.  Two layers in
//            front of the global atomics, each switchable:
//            wave  a sensor's neighbouring records are often one voxel's: a run of consecutive lanes with the same
//                  key is reduced with wave shuffles (a segmented sum over the run) and only its head goes on, with
//                  the run's sums, its length and its own index, the smallest of the run.
//            lds   the workgroup's own table in LDS, 1024 slots of the same 48 bytes (48 KiB: three workgroups, 12
//                  waves, a CU of 160 KiB), claimed and added to with LDS atomics, at most 16 probes; a head that
//                  finds no slot goes to global directly.  After the span one pass flushes every used slot, one
//                  global insertion per distinct voxel of the span.
//   count    the walk again: a point probes for its voxel's slot (no atomics); it is a writer iff it is the voxel's
//            first point and the count reaches min_points.  Per 256-point block the writers are counted from wave
//            ballots.  With `saved` the slot index of a writer (-1 for the others) is kept, one int32 per point.
//   scan     one workgroup per cloud: exclusive prefixes over the cloud's blocks in place, the total in counts[b].
//   scatter  a writer's rank is its block's prefix, plus the writers of the waves before its own (LDS), plus those of
//            the lanes before it in its wave's ballot.  It divides its slot's sums in float64 (one correctly rounded
//            division, then one rounding to float32; gfx950 has native fp64 and nothing here is built with relaxed
//            arithmetic) and stores the 16-byte record with one vector store.  With `saved` it reads no point at all;
//            without it loads the point and probes again.
//
// No workgroup waits on another in any launch.  Only integer atomics are used and the ranks come from prefixes, so no
// output depends on the order blocks run in; the reset belongs to the launch, so a relaunch or a graph replay gives the
// same bytes.  Nothing is allocated, no hipMemset is used, and every store is a whole-word or vector store.
//
// The arithmetic is the float32 definition, every operation rounded on its own: contraction to FMA is switched off
// for this file, division is IEEE.
#include "tca_cloud_load.h"
#include "tca_common.h"

#include <cmath>

#pragma clang fp contract(off)

using namespace tca;

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxFrames = 64;
constexpr int kMaxPoints = 1 << 24;
constexpr int kSpanBlocks = 8;     // 256-point blocks of one workgroup's span
constexpr int kLdsSlots = 1024;    // of the workgroup's table
constexpr int kLdsProbes = 16;
constexpr int kBias = 1 << 20;
constexpr unsigned long long kEmptyKey = ~0ull;
constexpr int kNoPoint = 0x7FFFFFFF;

struct Slot {  // 48 bytes, 16-byte aligned
  unsigned long long key;
  unsigned long long sum[4];  // x, y, z, intensity: two's complement
  int count, first;
};
static_assert(sizeof(Slot) == 48, "a slot is 48 bytes");

struct VoxelArgs {
  int step;
  int off[4];  // x, y, z, intensity (-1: none)
  int fast;    // tca_cloud_load.h
  int min_pts, max_n;
  float leaf[3];
  int n[kMaxFrames];         // the points of cloud b the host knows
  int pt_off[kMaxFrames];    // the points before cloud b: its first record in `out`, its first int32 in `memo`
  int mask[kMaxFrames];      // slots[b] - 1
  long slot_off[kMaxFrames]; // the slots before cloud b's table
};

// Quad i of a run of empty slots (a slot is three quads): the empty key, zero sums and count, no first point.
__device__ __forceinline__ uint4 empty_quad(long i) {
  const int part = (int)(i % 3);
  return part == 0 ? make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u)
       : part == 1 ? make_uint4(0u, 0u, 0u, 0u) : make_uint4(0u, 0u, 0u, (unsigned)kNoPoint);
}

__global__ void __launch_bounds__(kBlock) voxel_reset_kernel(uint4* __restrict__ table, long n_quads) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i < n_quads) table[i] = empty_quad(i);
}

struct Point {
  unsigned long long key;  // kEmptyKey: not valid
  long long q[4];
};

// Point i of the cloud at foff: its key and the integers it adds.  A record outside the buffer is not read.
__device__ __forceinline__ Point load_point(const uint8_t* __restrict__ data, long data_bytes, long foff, long i,
                                            int n_pts, const VoxelArgs& a, int path, bool want_q) {
  Point p;
  p.key = kEmptyKey;
  p.q[0] = p.q[1] = p.q[2] = p.q[3] = 0;
  const long at = foff + i * a.step;
  if (!(i < n_pts && foff >= 0 && foff <= data_bytes && at + a.step <= data_bytes)) return p;
  uint32_t raw[4] = {0u, 0u, 0u, 0u};
  cloud_load_fields(data + at, a.off, path, raw);
  if (a.off[3] < 0) raw[3] = 0u;  // (the 16-byte path loads whatever lies at byte 12)
  const float v[3] = {__uint_as_float(raw[0]), __uint_as_float(raw[1]), __uint_as_float(raw[2])};
  // a NaN compares false, an infinity is too large
  if (!(fabsf(v[0]) <= 512.f && fabsf(v[1]) <= 512.f && fabsf(v[2]) <= 512.f)) return p;
  unsigned long long key = 0ull;
#pragma unroll
  for (int j = 2; j >= 0; --j) {
    const int idx = (int)floorf(v[j] / a.leaf[j]);  // |idx| <= 51200
    key = (key << 21) | (unsigned long long)(idx + kBias);
  }
  p.key = key;
  if (want_q) {
#pragma unroll
    for (int j = 0; j < 3; ++j) p.q[j] = (long long)rintf(v[j] * 65536.f);  // the product is exact
    const float in = __uint_as_float(raw[3]);
    const float c = in != in ? 0.f : fminf(fmaxf(in, -65536.f), 65536.f);
    p.q[3] = (long long)rintf(c * 4096.f);
  }
  return p;
}

__device__ __forceinline__ unsigned hash_of(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (unsigned)k;
}

// Find or claim `key` in a cloud's table and add to it.  mask + 1 slots >= the cloud's points: the loop ends.
__device__ __forceinline__ void global_insert(Slot* __restrict__ tab, int mask, unsigned long long key,
                                              const long long (&q)[4], int count, int first) {
  unsigned h = hash_of(key) & (unsigned)mask;
  for (int probe = 0; probe <= mask; ++probe, h = (h + 1u) & (unsigned)mask) {
    Slot* s = tab + h;
    unsigned long long seen = s->key;  // (a key never changes once it is set)
    if (seen == kEmptyKey) seen = atomicCAS(&s->key, kEmptyKey, key);
    if (seen == kEmptyKey || seen == key) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (q[j] != 0) atomicAdd(&s->sum[j], (unsigned long long)q[j]);
      atomicAdd(&s->count, count);
      atomicMin(&s->first, first);
      return;
    }
  }
}

// The slot of `key` in a cloud's table after the insert pass, -1 if it is not there (it always is).
__device__ __forceinline__ int global_find(const Slot* __restrict__ tab, int mask, unsigned long long key) {
  unsigned h = hash_of(key) & (unsigned)mask;
  for (int probe = 0; probe <= mask; ++probe, h = (h + 1u) & (unsigned)mask) {
    const unsigned long long seen = tab[h].key;
    if (seen == key) return (int)h;
    if (seen == kEmptyKey) return -1;
  }
  return -1;
}

// The run of consecutive lanes with this lane's key (kEmptyKey: no run): the lane's position in it and its length.
__device__ __forceinline__ void wave_run64(unsigned long long key, int* pos, int* len) {
  const int lane = threadIdx.x & 63;
  const unsigned long long prev = __shfl_up(key, 1, 64);
  const bool head = key != kEmptyKey && (lane == 0 || prev != key);
  const unsigned long long brk = __ballot(key == kEmptyKey || head);  // every run starts at a break
  const unsigned long long after = lane == 63 ? 0ull : (brk >> (lane + 1));
  const int rest = after ? (__builtin_ctzll(after) + 1) : (64 - lane);  // lanes from this one to the run's end
  const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
  *pos = (brk & upto) ? lane - (63 - __builtin_clzll(brk & upto)) : 0;
  *len = *pos + rest;
}

template <bool kWave, bool kLds>
__global__ void __launch_bounds__(kBlock) voxel_insert_kernel(
    const uint8_t* __restrict__ data, long data_bytes, const long* __restrict__ frame_off,
    const int* __restrict__ frame_n, VoxelArgs a, Slot* __restrict__ table) {
  extern __shared__ uint4 lds_raw[];  // kLds: kLdsSlots slots
  Slot* mine = reinterpret_cast<Slot*>(lds_raw);

  const int b = blockIdx.y;
  const int n_pts = min(max(frame_n[b], 0), a.n[b]);
  const long span0 = (long)blockIdx.x * kSpanBlocks * kBlock;
  if (span0 >= n_pts) return;  // the whole workgroup: nothing of this cloud is its own
  const long foff = frame_off[b];
  const int path = cloud_frame_path(a.fast, foff);
  Slot* tab = table + a.slot_off[b];
  const int mask = a.mask[b];

  if (kLds) {
    for (int i = threadIdx.x; i < 3 * kLdsSlots; i += kBlock) lds_raw[i] = empty_quad(i);
    __syncthreads();
  }

  for (int k = 0; k < kSpanBlocks; ++k) {  // (the same trips for every lane of a wave)
    const long i = span0 + (long)k * kBlock + threadIdx.x;
    if (span0 + (long)k * kBlock >= n_pts) break;
    Point p = load_point(data, data_bytes, foff, i, n_pts, a, path, true);
    int count = 1;
    bool go = p.key != kEmptyKey;
    if (kWave) {
      int pos, len;
      wave_run64(p.key, &pos, &len);
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {  // a segmented sum: lane `pos` of a run gathers [pos, pos + 2 o)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const long long t = __shfl_down(p.q[j], o, 64);
          if (pos + o < len) p.q[j] += t;
        }
      }
      go = go && pos == 0;
      count = len;
    }
    if (!go) continue;
    bool done = false;
    if (kLds) {
      unsigned h = hash_of(p.key) & (kLdsSlots - 1);
      for (int probe = 0; probe < kLdsProbes && !done; ++probe, h = (h + 1u) & (kLdsSlots - 1)) {
        Slot* s = mine + h;
        unsigned long long seen = s->key;
        if (seen == kEmptyKey) seen = atomicCAS(&s->key, kEmptyKey, p.key);
        if (seen == kEmptyKey || seen == p.key) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (p.q[j] != 0) atomicAdd(&s->sum[j], (unsigned long long)p.q[j]);
          atomicAdd(&s->count, count);
          atomicMin(&s->first, (int)i);
          done = true;
        }
      }
    }
    if (!done) global_insert(tab, mask, p.key, p.q, count, (int)i);
  }

  if (kLds) {
    __syncthreads();
    for (int i = threadIdx.x; i < kLdsSlots; i += kBlock) {
      const Slot* s = mine + i;
      if (s->key == kEmptyKey) continue;
      const long long q[4] = {(long long)s->sum[0], (long long)s->sum[1], (long long)s->sum[2], (long long)s->sum[3]};
      global_insert(tab, mask, s->key, q, s->count, s->first);
    }
  }
}

// blocks: int32[B][nblk + 1] (nblk = ceil(max_n / 256)): per block its writers.
__global__ void __launch_bounds__(kBlock) voxel_count_kernel(
    const uint8_t* __restrict__ data, long data_bytes, const long* __restrict__ frame_off,
    const int* __restrict__ frame_n, VoxelArgs a, const Slot* __restrict__ table, int saved,
    int* __restrict__ blocks, int* __restrict__ memo) {
  __shared__ int w_cnt[kWaves];
  const int b = blockIdx.y;
  const int n_pts = min(max(frame_n[b], 0), a.n[b]);
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if ((long)blockIdx.x * kBlock >= n_pts) return;
  const long foff = frame_off[b];
  const Slot* tab = table + a.slot_off[b];
  const int nblk = (a.max_n + kBlock - 1) / kBlock;

  const Point p = load_point(data, data_bytes, foff, i, n_pts, a, cloud_frame_path(a.fast, foff), false);
  int slot = -1;
  if (p.key != kEmptyKey) {
    slot = global_find(tab, a.mask[b], p.key);
    if (slot >= 0 && !(tab[slot].first == (int)i && tab[slot].count >= a.min_pts)) slot = -1;
  }
  if (saved && i < n_pts) memo[a.pt_off[b] + i] = slot;
  const unsigned long long w = __ballot(slot >= 0);
  if ((threadIdx.x & 63) == 0) w_cnt[threadIdx.x >> 6] = __popcll(w);
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
    for (int k = 0; k < kWaves; ++k) n += w_cnt[k];
    blocks[(long)b * (nblk + 1) + blockIdx.x] = n;
  }
}

// One workgroup per cloud: the block counts become exclusive prefixes in place; the total goes into counts[b].
__global__ void __launch_bounds__(kBlock) voxel_scan_kernel(const int* __restrict__ frame_n, VoxelArgs a,
                                                            int* __restrict__ blocks, int* __restrict__ counts) {
  __shared__ int sum[kBlock];
  const int b = blockIdx.x, t = threadIdx.x;
  const int nblk = (a.max_n + kBlock - 1) / kBlock;
  const int n_blocks = (min(max(frame_n[b], 0), a.n[b]) + kBlock - 1) / kBlock;
  int* mine = blocks + (long)b * (nblk + 1);
  const int chunk = (n_blocks + kBlock - 1) / kBlock;
  const int lo = min(t * chunk, n_blocks), hi = min(lo + chunk, n_blocks);
  int own = 0;
  for (int k = lo; k < hi; ++k) own += mine[k];
  sum[t] = own;
  __syncthreads();
  for (int o = 1; o < kBlock; o <<= 1) {  // inclusive, over the threads' chunks
    const int v = t >= o ? sum[t - o] : 0;
    __syncthreads();
    sum[t] += v;
    __syncthreads();
  }
  int run = sum[t] - own;
  for (int k = lo; k < hi; ++k) {
    const int c = mine[k];
    mine[k] = run;
    run += c;
  }
  if (t == kBlock - 1) counts[b] = sum[t];
}

__device__ __forceinline__ float mean_of(unsigned long long sum, int n, int shift) {
  return (float)((double)(long long)sum / (double)((long long)n << shift));
}

template <bool kSaved>
__global__ void __launch_bounds__(kBlock) voxel_scatter_kernel(
    const uint8_t* __restrict__ data, long data_bytes, const long* __restrict__ frame_off,
    const int* __restrict__ frame_n, VoxelArgs a, const Slot* __restrict__ table, const int* __restrict__ blocks,
    const int* __restrict__ memo, uint4* __restrict__ out, long out_records) {
  __shared__ int w_cnt[kWaves];
  const int b = blockIdx.y;
  const int n_pts = min(max(frame_n[b], 0), a.n[b]);
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if ((long)blockIdx.x * kBlock >= n_pts) return;
  const Slot* tab = table + a.slot_off[b];
  const int nblk = (a.max_n + kBlock - 1) / kBlock;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;

  int slot = -1;
  if (kSaved) {
    if (i < n_pts) slot = memo[a.pt_off[b] + i];
    if (slot > a.mask[b]) slot = -1;  // (never: the count pass wrote it)
  } else {
    const long foff = frame_off[b];
    const Point p = load_point(data, data_bytes, foff, i, n_pts, a, cloud_frame_path(a.fast, foff), false);
    if (p.key != kEmptyKey) {
      slot = global_find(tab, a.mask[b], p.key);
      if (slot >= 0 && !(tab[slot].first == (int)i && tab[slot].count >= a.min_pts)) slot = -1;
    }
  }
  const unsigned long long w = __ballot(slot >= 0);
  if (lane == 0) w_cnt[wid] = __popcll(w);
  __syncthreads();
  if (slot < 0) return;
  int rank = blocks[(long)b * (nblk + 1) + blockIdx.x] + __popcll(w & ((1ull << lane) - 1ull));
  for (int k = 0; k < wid; ++k) rank += w_cnt[k];
  const Slot* s = tab + slot;
  const int n = s->count;
  uint4 rec;
  rec.x = __float_as_uint(mean_of(s->sum[0], n, 16));
  rec.y = __float_as_uint(mean_of(s->sum[1], n, 16));
  rec.z = __float_as_uint(mean_of(s->sum[2], n, 16));
  rec.w = __float_as_uint(mean_of(s->sum[3], n, 12));
  const long to = (long)a.pt_off[b] + rank;
  // a record of the cloud's own region (rank < its points); checked against the output's size all the same
  if (rank >= 0 && rank < n_pts && to < out_records) out[to] = rec;
}

}  // namespace

// data: device bytes, data_bytes of them (no record outside is read); frame_off long[B] (bytes) / frame_n int[B]:
// device; ns int[B], slots int[B]: HOST (read here, before the launches): the points of every cloud (the kernels
// clamp frame_n to them) and its table's size, a power of two at or above max(ns[b], 2).  Offsets of x, y, z and
// intensity (-1: none) in a record of FLOAT32 fields; leaf_*: float32(leaf) per axis, within 0.01..100; a voxel is kept
// from min_points points.  wave: 1, runs of equal voxels of a wave are reduced first; lds: 1, a workgroup gathers its
// span in an LDS table; saved: 1, the scatter reads the slots the count pass kept in memo (0 / 0 / 0: measurements).
// Workspace, reset here on the stream where it must be: table 48 bytes * sum(slots), 16-byte aligned; memo int32
// [sum(ns)]; blocks int32[B][ceil(max(ns) / 256) + 1].  out: 16-byte records, cloud b's from record sum(ns[:b]), at
// most ns[b] of them, out_bytes >= 16 * sum(ns), 16-byte aligned; counts int32[B]: the records of every cloud.  A
// buffer shorter than that, or misaligned, is refused, and nothing is launched.
TCA_API int tca_voxel_downsample(const void* data, long data_bytes, const long* frame_off, const int* frame_n,
                                 const int* ns, const int* slots, int batch, int point_step, int off_x, int off_y,
                                 int off_z, int off_i, float leaf_x, float leaf_y, float leaf_z, int min_points,
                                 int wave, int lds, int saved, void* table, long table_bytes, void* memo,
                                 long memo_bytes, void* blocks, long blocks_bytes, void* out, long out_bytes,
                                 void* counts, hipStream_t stream) {
  if (batch < 1 || batch > kMaxFrames || point_step <= 0 || data_bytes < 0 || data_bytes >= 0x80000000L ||
      min_points < 1 || ns == nullptr || slots == nullptr)
    return (int)hipErrorInvalidValue;
  if ((wave != 0 && wave != 1) || (lds != 0 && lds != 1) || (saved != 0 && saved != 1))
    return (int)hipErrorInvalidValue;
  const float leaf[3] = {leaf_x, leaf_y, leaf_z};
  for (float l : leaf)
    if (!(l >= 0.01f && l <= 100.f)) return (int)hipErrorInvalidValue;  // (a NaN compares false)
  VoxelArgs a;
  long n_sum = 0, slot_sum = 0;
  int max_n = 0;
  for (int b = 0; b < batch; ++b) {
    const int n = ns[b], s = slots[b];
    if (n < 0 || n > kMaxPoints || s < 2 || s < n || (s & (s - 1)) != 0) return (int)hipErrorInvalidValue;
    a.n[b] = n;
    a.mask[b] = s - 1;
    a.pt_off[b] = (int)n_sum;
    a.slot_off[b] = slot_sum;
    n_sum += n;
    slot_sum += s;
    max_n = n > max_n ? n : max_n;
    if (n_sum * point_step > data_bytes) return (int)hipErrorInvalidValue;  // (so n_sum < 2^31)
  }
  const int nblk = (max_n + kBlock - 1) / kBlock;
  if (table_bytes < 48 * slot_sum || memo_bytes < 4 * n_sum || blocks_bytes < 4L * batch * (nblk + 1) ||
      out_bytes < 16 * n_sum)
    return (int)hipErrorInvalidValue;
  if (frame_off == nullptr || frame_n == nullptr || table == nullptr || memo == nullptr || blocks == nullptr ||
      out == nullptr || counts == nullptr || (max_n > 0 && data == nullptr))
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)table & 15) != 0 || ((uintptr_t)out & 15) != 0 || ((uintptr_t)memo & 3) != 0 ||
      ((uintptr_t)blocks & 3) != 0 || ((uintptr_t)counts & 3) != 0 || ((uintptr_t)frame_off & 7) != 0 ||
      ((uintptr_t)frame_n & 3) != 0)
    return (int)hipErrorInvalidValue;
  a.step = point_step;
  a.off[0] = off_x; a.off[1] = off_y; a.off[2] = off_z; a.off[3] = off_i;
  a.fast = cloud_fast_path(data, point_step, a.off, true);
  if (a.fast < 0) return (int)hipErrorInvalidValue;
  a.min_pts = min_points; a.max_n = max_n;
  a.leaf[0] = leaf_x; a.leaf[1] = leaf_y; a.leaf[2] = leaf_z;

  const uint8_t* in = (const uint8_t*)data;
  Slot* tab = (Slot*)table;
  if (max_n > 0) {
    const long quads = 3 * slot_sum;
    voxel_reset_kernel<<<(unsigned)((quads + kBlock - 1) / kBlock), kBlock, 0, stream>>>((uint4*)table, quads);
    if (int e = (int)hipGetLastError()) return e;
    const int span = kSpanBlocks * kBlock;
    const dim3 grid((max_n + span - 1) / span, batch);
    const size_t bytes = lds ? (size_t)kLdsSlots * sizeof(Slot) : 0;
    if (wave && lds)
      voxel_insert_kernel<true, true><<<grid, kBlock, bytes, stream>>>(in, data_bytes, frame_off, frame_n, a, tab);
    else if (wave)
      voxel_insert_kernel<true, false><<<grid, kBlock, bytes, stream>>>(in, data_bytes, frame_off, frame_n, a, tab);
    else if (lds)
      voxel_insert_kernel<false, true><<<grid, kBlock, bytes, stream>>>(in, data_bytes, frame_off, frame_n, a, tab);
    else
      voxel_insert_kernel<false, false><<<grid, kBlock, bytes, stream>>>(in, data_bytes, frame_off, frame_n, a, tab);
    if (int e = (int)hipGetLastError()) return e;
    voxel_count_kernel<<<dim3(nblk, batch), kBlock, 0, stream>>>(in, data_bytes, frame_off, frame_n, a, tab, saved,
                                                                 (int*)blocks, (int*)memo);
    if (int e = (int)hipGetLastError()) return e;
  }
  voxel_scan_kernel<<<batch, kBlock, 0, stream>>>(frame_n, a, (int*)blocks, (int*)counts);
  if (max_n > 0) {
    if (int e = (int)hipGetLastError()) return e;
    if (saved)
      voxel_scatter_kernel<true><<<dim3(nblk, batch), kBlock, 0, stream>>>(
          in, data_bytes, frame_off, frame_n, a, tab, (const int*)blocks, (const int*)memo, (uint4*)out, n_sum);
    else
      voxel_scatter_kernel<false><<<dim3(nblk, batch), kBlock, 0, stream>>>(
          in, data_bytes, frame_off, frame_n, a, tab, (const int*)blocks, (const int*)memo, (uint4*)out, n_sum);
  }
  TCA_LAUNCH_CHECK();
}
