// K30 — the cloud split into ground and obstacles: the input records that stand above the estimated
// ground, and those at or below it, each compacted in input order, byte for byte.
//
// Batched over B <= 64 clouds that share one field layout.  Raw PointCloud2 bytes are read in
// place (tca_cloud_load.h).  The grid is polar: S sectors (the laser scan's pseudo-angle against a
// host-built table of S + 1 non-decreasing edges, K29) times nr rings of `cell` metres; heights are
// integers in units of 1/1024 m (ops/ground.py has the definition).
//
//   reset     the cell plane int32[B][nr][S] is set to EMPTY = INT32_MAX.  Ring-major: the sweep's
//             lanes, one sector each, read consecutive addresses.
//   cells     blockIdx.y = cloud.  A workgroup keeps the S + 1 edges in LDS ((S + 1) * 4 bytes,
//             16 KiB at most), walks 256-point blocks of its cloud with a stride of gridDim.x
//             blocks, finds each valid point's sector by binary search in LDS (13 steps at most)
//             and does one global integer atomicMin of the point's height into its cell.  A cloud
//             spreads over tens of thousands of cells, so the lanes of a wave rarely meet.
//   sweep     one thread per (cloud, sector) walks the nr rings outwards and overwrites the cell
//             minima M with the ground estimate G in place.  The loads do not depend on the running
//             state: eight are issued ahead of the eight dependent steps.
//   classify  the walk of `cells` again: the class of every point against G (0 dropped, 1 ground,
//             2 obstacle) and, per 256-point block, the number of obstacles and of ground points
//             from wave ballots.  With `saved` the class is also stored, one byte per record.
//   scan      one workgroup per cloud: exclusive prefixes over the cloud's blocks in place, the
//             totals behind them and in `counts`.
//   scatter   the walk again.  A record's rank is its block's prefix, plus the counts of the waves
//             before its own (LDS), plus the lanes before it in its wave's ballot.  The class comes
//             from the saved byte or is computed again.  The record's point_step bytes are moved
//             with 16-byte, dword or byte loads and stores, whichever source, destination and step
//             allow.
//
// No workgroup waits on another in any launch: the prefixes come from a launch of their own, not
// from a look-back.  Only integer atomics are used and the ranks come from prefixes, so no output
// depends on the order blocks run in.  Everything a launch reads it has written itself, so a
// relaunch or a graph replay gives the same bytes.
//
// Output.  `out` mirrors the staged input: cloud b's slot starts at out + frame_off[b] and holds
// frame_n[b] records; obstacles fill records [0, n_obs), ground fills [n - n_gnd, n), the bytes
// between are not written.  `want` (1 obstacles, 2 ground) says which of the two regions and counts
// are written; the other stays untouched.
//
// The arithmetic is the float32 definition of ops/ground.py, every operation rounded on its own:
// contraction to FMA is switched off for this file, division and square root are IEEE.
#include "tca_cloud_load.h"
#include "tca_common.h"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

using namespace tca;

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxFrames = 64;
constexpr int kMaxSectors = 4096;
constexpr int kMaxRings = 512;
constexpr int kMaxPlane = 1 << 24;
constexpr int kQLimit = 1 << 21;
constexpr int kEmpty = 0x7FFFFFFF;

struct GroundArgs {
  int step;
  int off[4];  // x, y, z, -1
  int fast;    // tca_cloud_load.h
  int S, nr;
  int max_n;
  float c32, r0;
  int h0, slope_q, noise_q, thick_q, top_q;
};

__global__ void __launch_bounds__(kBlock) ground_reset_kernel(int* __restrict__ plane, int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) plane[i] = kEmpty;
}

// Point i of the cloud at foff: is it valid, and if so its sector, ring and height.  A record
// outside the buffer is not read (not valid); *readable says whether it was.
__device__ __forceinline__ bool point_cell(const uint8_t* __restrict__ data, long data_bytes, long foff, long i,
                                           int n_pts, const GroundArgs& a, int path, const float* tab, int* sector,
                                           int* ring, int* zi, bool* readable) {
  const long at = foff + i * a.step;
  *readable = i < n_pts && foff >= 0 && foff <= data_bytes && at + a.step <= data_bytes;
  if (!*readable) return false;
  uint32_t raw[4] = {0u, 0u, 0u, 0u};
  cloud_load_fields(data + at, a.off, path, raw);
  const float x = __uint_as_float(raw[0]), y = __uint_as_float(raw[1]), z = __uint_as_float(raw[2]);

  // a NaN compares false
  if (!(fabsf(z) <= 512.f)) return false;
  const float r = sqrtf(x * x + y * y);
  const float d = r / a.c32;
  if (!(r >= a.r0 && d < (float)a.nr)) return false;
  const float s = fabsf(x) + fabsf(y);
  if (!(s != 0.f && s <= 3.402823466e+38f)) return false;  // zero, infinite or NaN
  const float q = copysignf(1.f - x / s, y);
  if (!(q >= tab[0] && q <= tab[a.S])) return false;

  int lo = 0, hi = a.S + 1;  // the number of edges <= q: searchsorted(table, q, "right")
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tab[mid] <= q) lo = mid + 1; else hi = mid;
  }
  // q >= t0: lo >= 1; q == tS: sector S - 1; the clamp only matters for a table that is not sorted
  *sector = min(max(lo - 1, 0), a.S - 1);
  *ring = min((int)d, a.nr - 1);  // d < nr: the clamp changes nothing
  *zi = (int)rintf(z * 1024.f);
  return true;
}

__global__ void __launch_bounds__(kBlock) ground_cells_kernel(
    const uint8_t* __restrict__ data, long data_bytes, const long* __restrict__ frame_off,
    const int* __restrict__ frame_n, const float* __restrict__ table, GroundArgs a, int* __restrict__ plane) {
  extern __shared__ float tab[];  // S + 1 edges

  const int b = blockIdx.y;
  const int n_pts = min(frame_n[b], a.max_n);
  const int n_blocks = (n_pts + kBlock - 1) / kBlock;
  if ((int)blockIdx.x >= n_blocks) return;  // the whole workgroup: nothing of this cloud is its own
  const long foff = frame_off[b];
  const int path = cloud_frame_path(a.fast, foff);
  int* cells = plane + (long)b * a.nr * a.S;

  for (int i = threadIdx.x; i <= a.S; i += kBlock) tab[i] = table[i];
  __syncthreads();

  for (int blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    int s, j, zi;
    bool readable;
    if (point_cell(data, data_bytes, foff, (long)blk * kBlock + threadIdx.x, n_pts, a, path, tab, &s, &j, &zi,
                   &readable))
      atomicMin(cells + (long)j * a.S + s, zi);
  }
}

__global__ void __launch_bounds__(kBlock) ground_sweep_kernel(int* __restrict__ plane, int batch, GroundArgs a) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= batch * a.S) return;
  const int b = t / a.S, s = t - b * a.S;
  int* p = plane + (long)b * a.nr * a.S + s;
  int g = a.h0, jg = -1;
  for (int j0 = 0; j0 < a.nr; j0 += 8) {
    int m[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) m[k] = j0 + k < a.nr ? p[(long)(j0 + k) * a.S] : kEmpty;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int j = j0 + k;
      if (j < a.nr) {
        if (m[k] != kEmpty) {
          const int allow = a.noise_q + a.slope_q * (j - jg);
          const int dz = m[k] - g;
          if ((dz < 0 ? -dz : dz) <= allow) { g = m[k]; jg = j; }
        }
        p[(long)j * a.S] = g;
      }
    }
  }
}

__device__ __forceinline__ int class_of(int zi, int g, const GroundArgs& a) {
  const int h = zi - g;
  return h <= a.thick_q ? 1 : h <= a.top_q ? 2 : 0;
}

// blocks: int32[B][nblk + 1][2] (nblk = ceil(max_n / 256)): per block (obstacles, ground).
template <bool kSaved>
__global__ void __launch_bounds__(kBlock) ground_classify_kernel(
    const uint8_t* __restrict__ data, long data_bytes, const long* __restrict__ frame_off,
    const int* __restrict__ frame_n, const float* __restrict__ table, GroundArgs a, const int* __restrict__ plane,
    int* __restrict__ blocks, uint8_t* __restrict__ cls) {
  extern __shared__ float tab[];
  __shared__ int w_cnt[kWaves][2];

  const int b = blockIdx.y;
  const int n_pts = min(frame_n[b], a.max_n);
  const int n_blocks = (n_pts + kBlock - 1) / kBlock;
  if ((int)blockIdx.x >= n_blocks) return;
  const long foff = frame_off[b];
  const int path = cloud_frame_path(a.fast, foff);
  const int* G = plane + (long)b * a.nr * a.S;
  int* mine = blocks + (long)b * ((a.max_n + kBlock - 1) / kBlock + 1) * 2;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;

  for (int i = threadIdx.x; i <= a.S; i += kBlock) tab[i] = table[i];
  __syncthreads();

  for (int blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {  // (the same trips for every lane)
    const long i = (long)blk * kBlock + threadIdx.x;
    int s, j, zi, c = 0;
    bool readable;
    if (point_cell(data, data_bytes, foff, i, n_pts, a, path, tab, &s, &j, &zi, &readable))
      c = class_of(zi, G[(long)j * a.S + s], a);
    if (kSaved && readable) cls[(foff + i * a.step) / a.step] = (uint8_t)c;
    const unsigned long long obs = __ballot(c == 2), gnd = __ballot(c == 1);
    if (lane == 0) { w_cnt[wid][0] = __popcll(obs); w_cnt[wid][1] = __popcll(gnd); }
    __syncthreads();
    if (threadIdx.x < 2) {
      int n = 0;
      for (int w = 0; w < kWaves; ++w) n += w_cnt[w][threadIdx.x];
      mine[2 * blk + threadIdx.x] = n;
    }
    __syncthreads();  // w_cnt is free again
  }
}

// One workgroup per cloud: the block counts become exclusive prefixes in place; the totals go
// behind them (entry nblk) and, for what is wanted, into counts[b].
__global__ void __launch_bounds__(kBlock) ground_scan_kernel(const int* __restrict__ frame_n, int max_n, int want,
                                                             int* __restrict__ blocks, int* __restrict__ counts) {
  __shared__ int sum[2][kBlock];
  const int b = blockIdx.x, t = threadIdx.x;
  const int nblk = (max_n + kBlock - 1) / kBlock;
  const int n_blocks = (min(frame_n[b], max_n) + kBlock - 1) / kBlock;
  int* mine = blocks + (long)b * (nblk + 1) * 2;
  const int chunk = (n_blocks + kBlock - 1) / kBlock;
  const int lo = min(t * chunk, n_blocks), hi = min(lo + chunk, n_blocks);
  int own[2] = {0, 0};
  for (int k = lo; k < hi; ++k) { own[0] += mine[2 * k]; own[1] += mine[2 * k + 1]; }
  sum[0][t] = own[0];
  sum[1][t] = own[1];
  __syncthreads();
  for (int o = 1; o < kBlock; o <<= 1) {  // inclusive, over the threads' chunks
    const int v0 = t >= o ? sum[0][t - o] : 0, v1 = t >= o ? sum[1][t - o] : 0;
    __syncthreads();
    sum[0][t] += v0;
    sum[1][t] += v1;
    __syncthreads();
  }
  int run[2] = {sum[0][t] - own[0], sum[1][t] - own[1]};
  for (int k = lo; k < hi; ++k) {
    const int c0 = mine[2 * k], c1 = mine[2 * k + 1];
    mine[2 * k] = run[0];
    mine[2 * k + 1] = run[1];
    run[0] += c0;
    run[1] += c1;
  }
  if (t == kBlock - 1) {
    mine[2 * nblk] = sum[0][t];
    mine[2 * nblk + 1] = sum[1][t];
    if (want & 1) counts[2 * b] = sum[0][t];
    if (want & 2) counts[2 * b + 1] = sum[1][t];
  }
}

__device__ __forceinline__ void copy_record(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int step) {
  const uintptr_t m = (uintptr_t)src | (uintptr_t)dst | (uintptr_t)step;
  if ((m & 15) == 0) {
    for (int k = 0; k < step; k += 16) *reinterpret_cast<uint4*>(dst + k) = *reinterpret_cast<const uint4*>(src + k);
  } else if ((m & 3) == 0) {
    for (int k = 0; k < step; k += 4)
      *reinterpret_cast<uint32_t*>(dst + k) = *reinterpret_cast<const uint32_t*>(src + k);
  } else {
    for (int k = 0; k < step; ++k) dst[k] = src[k];
  }
}

template <bool kSaved>
__global__ void __launch_bounds__(kBlock) ground_scatter_kernel(
    const uint8_t* __restrict__ data, long data_bytes, const long* __restrict__ frame_off,
    const int* __restrict__ frame_n, const float* __restrict__ table, GroundArgs a, const int* __restrict__ plane,
    const int* __restrict__ blocks, const uint8_t* __restrict__ cls, int want, uint8_t* __restrict__ out,
    long out_bytes) {
  extern __shared__ float tab[];
  __shared__ int w_cnt[kWaves][2];

  const int b = blockIdx.y;
  const int n_pts = min(frame_n[b], a.max_n);
  const int n_blocks = (n_pts + kBlock - 1) / kBlock;
  if ((int)blockIdx.x >= n_blocks) return;
  const long foff = frame_off[b];
  const int path = cloud_frame_path(a.fast, foff);
  const int* G = plane + (long)b * a.nr * a.S;
  const int nblk = (a.max_n + kBlock - 1) / kBlock;
  const int* mine = blocks + (long)b * (nblk + 1) * 2;
  const int first_gnd = n_pts - mine[2 * nblk + 1];  // the ground region ends the slot
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const unsigned long long before = (1ull << lane) - 1ull;

  if (!kSaved) {
    for (int i = threadIdx.x; i <= a.S; i += kBlock) tab[i] = table[i];
    __syncthreads();
  }

  for (int blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {  // (the same trips for every lane)
    const long i = (long)blk * kBlock + threadIdx.x;
    const long at = foff + i * a.step;
    int c = 0;
    if (kSaved) {
      if (i < n_pts && foff >= 0 && foff <= data_bytes && at + a.step <= data_bytes) c = cls[at / a.step];
    } else {
      int s, j, zi;
      bool readable;
      if (point_cell(data, data_bytes, foff, i, n_pts, a, path, tab, &s, &j, &zi, &readable))
        c = class_of(zi, G[(long)j * a.S + s], a);
    }
    const bool is_obs = c == 2 && (want & 1), is_gnd = c == 1 && (want & 2);
    const unsigned long long obs = __ballot(is_obs), gnd = __ballot(is_gnd);
    if (lane == 0) { w_cnt[wid][0] = __popcll(obs); w_cnt[wid][1] = __popcll(gnd); }
    __syncthreads();
    if (is_obs || is_gnd) {
      const int k = is_obs ? 0 : 1;
      int rank = mine[2 * blk + k] + __popcll((is_obs ? obs : gnd) & before);
      for (int w = 0; w < wid; ++w) rank += w_cnt[w][k];
      const long to = foff + (long)(is_obs ? rank : first_gnd + rank) * a.step;
      // a record of the cloud's slot in `out`; checked against the output's own size all the same
      if (rank >= 0 && to >= 0 && to + a.step <= out_bytes) copy_record(data + at, out + to, a.step);
    }
    __syncthreads();  // w_cnt is free again
  }
}

}  // namespace

// data: device bytes, data_bytes of them (no record outside is read); frame_off long[B] (bytes) / frame_n int[B]:
// device; max_n: the largest frame_n (host, sizes the grids and the block table); offsets of x, y, z in a record of
// FLOAT32 fields.  table: device float[sectors + 1], non-decreasing.  cell, range_min: float32(cell) and
// float32(range_min); h0 ... top_q: the integer constants of ops/ground.py in 1/1024 m.  want: 1 obstacles, 2 ground,
// 3 both.  saved: 1, the scatter reads the classes the count pass stored in cls; 0, it computes them again.
// Workspace: plane int32[B * rings * sectors], blocks int32[B][ceil(max_n / 256) + 1][2], cls data_bytes /
// point_step + 1 bytes.  out: out_bytes bytes laid out like data (every slot of frame_n records must lie inside: a
// record that would not is not written, though counted); counts int32[B][2] (obstacles, ground).
TCA_API int tca_ground_split(const void* data, long data_bytes, const long* frame_off, const int* frame_n, int batch,
                             int max_n, int point_step, int off_x, int off_y, int off_z, const float* table,
                             int sectors, int rings, float cell, float range_min, int h0, int slope_q, int noise_q,
                             int thick_q, int top_q, int want, int saved, void* plane, void* blocks, void* cls,
                             void* out, long out_bytes, void* counts, hipStream_t stream) {
  if (batch < 1 || batch > kMaxFrames || max_n < 0 || point_step <= 0 || data_bytes < 0 ||
      data_bytes >= 0x80000000L || out_bytes < 0 || out_bytes >= 0x80000000L)
    return (int)hipErrorInvalidValue;
  if (sectors < 1 || sectors > kMaxSectors || rings < 1 || rings > kMaxRings ||
      (long)batch * sectors * rings > kMaxPlane)
    return (int)hipErrorInvalidValue;
  if (want < 1 || want > 3 || (saved != 0 && saved != 1)) return (int)hipErrorInvalidValue;
  if (!std::isfinite(cell) || !(cell > 0.f) || !std::isfinite(range_min) || !(range_min >= 0.f))
    return (int)hipErrorInvalidValue;
  if (h0 < -kQLimit || h0 > kQLimit || slope_q < 0 || slope_q > 16384 || noise_q < 0 || noise_q > kQLimit ||
      thick_q < 0 || thick_q > kQLimit || top_q < 0 || top_q > kQLimit)
    return (int)hipErrorInvalidValue;
  if (table == nullptr || frame_off == nullptr || frame_n == nullptr || plane == nullptr || blocks == nullptr ||
      cls == nullptr || out == nullptr || counts == nullptr || (max_n > 0 && data == nullptr) || out == data)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)plane & 3) != 0 || ((uintptr_t)blocks & 3) != 0 || ((uintptr_t)counts & 3) != 0 ||
      ((uintptr_t)table & 3) != 0 || ((uintptr_t)frame_off & 7) != 0 || ((uintptr_t)frame_n & 3) != 0)
    return (int)hipErrorInvalidValue;
  GroundArgs a;
  a.step = point_step;
  a.off[0] = off_x; a.off[1] = off_y; a.off[2] = off_z; a.off[3] = -1;
  a.fast = cloud_fast_path(data, point_step, a.off, true);
  if (a.fast < 0) return (int)hipErrorInvalidValue;
  a.S = sectors; a.nr = rings; a.max_n = max_n;
  a.c32 = cell; a.r0 = range_min;
  a.h0 = h0; a.slope_q = slope_q; a.noise_q = noise_q; a.thick_q = thick_q; a.top_q = top_q;

  const uint8_t* in = (const uint8_t*)data;
  if (max_n > 0) {
    const int cells = batch * sectors * rings;  // <= 2^24
    ground_reset_kernel<<<(unsigned)((cells + kBlock - 1) / kBlock), kBlock, 0, stream>>>((int*)plane, cells);
    if (int e = (int)hipGetLastError()) return e;
    const int n_blocks = (max_n + kBlock - 1) / kBlock;
    // blocks per workgroup: the table's fill ((S + 1) / 256 passes) stays a fraction of the walk, as in K29
    const int k = std::min(32, std::max(4, sectors / 128));
    const dim3 grid((n_blocks + k - 1) / k, batch);
    const size_t lds = (size_t)(sectors + 1) * sizeof(float);
    ground_cells_kernel<<<grid, kBlock, lds, stream>>>(in, data_bytes, frame_off, frame_n, table, a, (int*)plane);
    if (int e = (int)hipGetLastError()) return e;
    ground_sweep_kernel<<<(unsigned)((batch * sectors + kBlock - 1) / kBlock), kBlock, 0, stream>>>((int*)plane,
                                                                                                   batch, a);
    if (int e = (int)hipGetLastError()) return e;
    if (saved)
      ground_classify_kernel<true><<<grid, kBlock, lds, stream>>>(in, data_bytes, frame_off, frame_n, table, a,
                                                                  (const int*)plane, (int*)blocks, (uint8_t*)cls);
    else
      ground_classify_kernel<false><<<grid, kBlock, lds, stream>>>(in, data_bytes, frame_off, frame_n, table, a,
                                                                   (const int*)plane, (int*)blocks, (uint8_t*)cls);
    if (int e = (int)hipGetLastError()) return e;
  }
  ground_scan_kernel<<<batch, kBlock, 0, stream>>>(frame_n, max_n, want, (int*)blocks, (int*)counts);
  if (max_n > 0) {
    if (int e = (int)hipGetLastError()) return e;
    const int n_blocks = (max_n + kBlock - 1) / kBlock;
    const int k = saved ? 4 : std::min(32, std::max(4, sectors / 128));
    const dim3 grid((n_blocks + k - 1) / k, batch);
    if (saved)
      ground_scatter_kernel<true><<<grid, kBlock, 0, stream>>>(in, data_bytes, frame_off, frame_n, table, a,
                                                               (const int*)plane, (const int*)blocks,
                                                               (const uint8_t*)cls, want, (uint8_t*)out, out_bytes);
    else
      ground_scatter_kernel<false><<<grid, kBlock, (size_t)(sectors + 1) * sizeof(float), stream>>>(
          in, data_bytes, frame_off, frame_n, table, a, (const int*)plane, (const int*)blocks, (const uint8_t*)cls,
          want, (uint8_t*)out, out_bytes);
  }
  TCA_LAUNCH_CHECK();
}
