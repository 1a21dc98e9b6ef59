// K26 — range camera detections from the LiDAR cloud: project every point into the image,
// and per pixel box take a depth quantile and the fixed-point mean of the points around it.
//
// Batched over B <= 64 clouds that share one field layout.  Raw PointCloud2 bytes are read in
// place (tca_cloud_load.h: 16-byte record, dwords or bytes, chosen from the alignment of the
// base pointer and of each frame's offset); the boxes are ragged (box_off[B + 1], at most 512
// per frame) rows (u0, v0, u1, v1) the host prepares, all NaN for a box that contains nothing.
// M = float32(P @ T) [3, 4] is the only calibration the device sees.
//
//   pass 1   one lane per point, blocks of 256; the frame's rows go through LDS in chunks of
//            kChunk and are read as broadcasts.  A hit adds 1 to hist[box][bin]; the lanes of
//            a wave that share a (box, bin) add once, with their number.
//   select   one wave per box scans its 512 bins: n, the quantile bin m, and the zeroed sums.
//   pass 2   the same walk; the hits within `window` bins of m add c and the three 64-bit
//            fixed-point sums, through LDS per block, then one global atomic per box and block.
//
// Every accumulation is an integer atomic, so no output depends on the order blocks run in.
// The arithmetic is the float32 definition of ops/range2d.py, every operation rounded on its
// own: contraction to FMA is switched off for this file.  No transcendental runs here.
#include "tca_cloud_load.h"
#include "tca_common.h"

#include <cmath>

#pragma clang fp contract(off)

using namespace tca;

namespace {

constexpr int kBlock = 256;
constexpr int kChunk = 128;      // boxes per LDS stage
constexpr int kBins = 512;       // NB of the definition
constexpr int kMaxFrames = 64;
constexpr int kMaxBoxes = 512;   // per frame
constexpr int kOutInts = 10;     // ints per output record: n, m, c, 0, then sx, sy, sz as int64
constexpr float kFixScale = 1024.f;
constexpr float kFixLimit = 1073741824.f;  // 2^30

struct RangeArgs {
  int step;
  int off[4];  // x, y, z, -1
  int fast;    // tca_cloud_load.h
  float m[12];
  float bin_w, min_depth;
  int window;
  int box_off[kMaxFrames + 1];
};

__device__ __forceinline__ int fix1024(float x) {
  float t = x * kFixScale;
  t = t > kFixLimit ? kFixLimit : (t < -kFixLimit ? -kFixLimit : t);
  return (int)rintf(t);  // v_rndne_f32: half to even
}

// PASS 1: hist[box][bin] += 1 per hit.  PASS 2: c and the sums of the hits near the box's m.
template <int PASS>
__global__ void __launch_bounds__(kBlock) range2d_points_kernel(
    const uint8_t* __restrict__ data, long data_bytes, const long* __restrict__ frame_off,
    const int* __restrict__ frame_n, RangeArgs a, const float4* __restrict__ table, int* __restrict__ hist,
    int* __restrict__ out) {
  __shared__ float4 s_row[kChunk];
  __shared__ int s_m[kChunk];
  __shared__ int s_c[kChunk];
  __shared__ unsigned long long s_sum[kChunk * 3];
  const int b = blockIdx.y;
  const int n = frame_n[b];
  if ((long)blockIdx.x * kBlock >= n) return;  // block-uniform: before any barrier
  const int k0 = a.box_off[b], k1 = a.box_off[b + 1];
  if (k1 <= k0) return;
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  const long foff = frame_off[b];
  const long at = foff + i * a.step;
  const bool live = i < n && foff >= 0 && at + a.step <= data_bytes;  // a record outside the buffer is not read

  uint32_t raw[4] = {0u, 0u, 0u, 0u};
  if (live) cloud_load_fields(data + at, a.off, cloud_frame_path(a.fast, foff), raw);
  const float x = __uint_as_float(raw[0]), y = __uint_as_float(raw[1]), z = __uint_as_float(raw[2]);

  const float w = ((a.m[8] * x + a.m[9] * y) + a.m[10] * z) + a.m[11];
  const float pa = ((a.m[0] * x + a.m[1] * y) + a.m[2] * z) + a.m[3];
  const float pb = ((a.m[4] * x + a.m[5] * y) + a.m[6] * z) + a.m[7];
  const float q = w / a.bin_w;
  // a NaN compares false; 0 <= q < kBins keeps the bin inside the histogram whatever min_depth is
  const bool visible = live && w >= a.min_depth && q >= 0.f && q < (float)kBins;
  if (!__syncthreads_or(visible ? 1 : 0)) return;  // block-uniform
  const int bin = visible ? (int)q : 0;            // truncation
  const float u = pa / w, v = pb / w;
  int fx = 0, fy = 0, fz = 0;
  if (PASS == 2 && visible) {
    fx = fix1024(x);
    fy = fix1024(y);
    fz = fix1024(z);
  }
  const int lane = threadIdx.x & 63;

  for (int c0 = k0; c0 < k1; c0 += kChunk) {
    const int nb = min(kChunk, k1 - c0);
    __syncthreads();  // the previous chunk is flushed
    if (threadIdx.x < nb) {
      s_row[threadIdx.x] = table[c0 + threadIdx.x];
      if (PASS == 2) {
        s_m[threadIdx.x] = out[(long)(c0 + threadIdx.x) * kOutInts + 1];
        s_c[threadIdx.x] = 0;
        s_sum[threadIdx.x * 3 + 0] = 0ull;
        s_sum[threadIdx.x * 3 + 1] = 0ull;
        s_sum[threadIdx.x * 3 + 2] = 0ull;
      }
    }
    __syncthreads();
    for (int j = 0; j < nb; ++j) {
      const float4 r = s_row[j];
      // closed edges; a NaN anywhere (point or row) compares false
      const bool in = visible && r.x <= u && u <= r.z && r.y <= v && v <= r.w;
      if (PASS == 1) {
        unsigned long long rem = __ballot(in);
        while (rem != 0ull) {  // wave-uniform
          const int lead = __ffsll((long long)rem) - 1;
          const int lb = __shfl(bin, lead, 64);
          const unsigned long long same = __ballot(in && bin == lb);
          if (lane == lead) atomicAdd(&hist[(long)(c0 + j) * kBins + lb], __popcll(same));
          rem &= ~same;
        }
      } else if (in) {
        const int m = s_m[j];
        const int d = bin - m;
        if (m >= 0 && d <= a.window && -d <= a.window) {
          atomicAdd(&s_c[j], 1);
          atomicAdd(&s_sum[j * 3 + 0], (unsigned long long)(long long)fx);
          atomicAdd(&s_sum[j * 3 + 1], (unsigned long long)(long long)fy);
          atomicAdd(&s_sum[j * 3 + 2], (unsigned long long)(long long)fz);
        }
      }
    }
    if (PASS == 2) {
      __syncthreads();
      if (threadIdx.x < nb && s_c[threadIdx.x] != 0) {
        int* o = out + (long)(c0 + threadIdx.x) * kOutInts;
        unsigned long long* os = reinterpret_cast<unsigned long long*>(o + 4);
        atomicAdd(o + 2, s_c[threadIdx.x]);
        atomicAdd(os + 0, s_sum[threadIdx.x * 3 + 0]);
        atomicAdd(os + 1, s_sum[threadIdx.x * 3 + 1]);
        atomicAdd(os + 2, s_sum[threadIdx.x * 3 + 2]);
      }
    }
  }
}

// One wave per box: n = the histogram's total, m = the smallest bin whose cumulated count
// reaches pct percent of n (-1 below min_points); the record's c and sums are zeroed.
__global__ void __launch_bounds__(kBlock) range2d_select_kernel(const int* __restrict__ hist, int n_boxes, int pct,
                                                                int min_points, int* __restrict__ out) {
  const int k = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (k >= n_boxes) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  constexpr int kPer = kBins / 64;
  const int4* h = reinterpret_cast<const int4*>(hist + (long)k * kBins + lane * kPer);
  const int4 h0 = h[0], h1 = h[1];
  const int v[kPer] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
  int local = 0;
#pragma unroll
  for (int t = 0; t < kPer; ++t) local += v[t];
  const int incl = wave_incl_sum(local);
  const int n = __shfl(incl, 63, 64);
  const long long need = (long long)n * pct;
  long long cum = incl - local;
  int m = kBins;
#pragma unroll
  for (int t = 0; t < kPer; ++t) {
    cum += v[t];
    if (m == kBins && cum * 100 >= need) m = lane * kPer + t;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o, 64));
  if (n < min_points || m >= kBins) m = -1;
  if (lane < kOutInts) out[(long)k * kOutInts + lane] = lane == 0 ? n : lane == 1 ? m : 0;
}

}  // namespace

// data: device bytes, data_bytes of them (no record outside is read); frame_off long[B] (bytes) / frame_n int[B]:
// device; max_n: the largest frame_n (host, sizes the grid); offsets of x, y, z in a record of FLOAT32 fields.
// box_off int[B + 1] and m float[12] (row-major [3, 4]): HOST, copied into the launch.  table float[K, 4]: device,
// 16-B aligned.  hist: K * 512 ints of workspace, zeroed here on the stream.  out: K records of 40 B
// (int n, m, c, 0; int64 sx, sy, sz), 8-B aligned.
TCA_API int tca_range2d(const void* data, long data_bytes, const long* frame_off, const int* frame_n, int batch,
                        int max_n, int point_step, int off_x, int off_y, int off_z, const int* box_off,
                        const float* table, const float* m, float bin_w, float min_depth, int pct, int min_points,
                        int window, int* hist, void* out, hipStream_t stream) {
  if (batch < 0 || batch > kMaxFrames || max_n < 0 || point_step <= 0 || data_bytes < 0 ||
      data_bytes >= 0x80000000L)
    return (int)hipErrorInvalidValue;
  if (box_off == nullptr || m == nullptr || frame_off == nullptr || frame_n == nullptr)
    return (int)hipErrorInvalidValue;
  if (pct < 1 || pct > 100 || min_points < 1 || window < 0 || !std::isfinite(bin_w) || !(bin_w > 0.f) ||
      !std::isfinite(min_depth))
    return (int)hipErrorInvalidValue;
  RangeArgs a;
  a.step = point_step;
  a.off[0] = off_x; a.off[1] = off_y; a.off[2] = off_z; a.off[3] = -1;
  a.fast = cloud_fast_path(data, point_step, a.off, true);
  if (a.fast < 0) return (int)hipErrorInvalidValue;
  if (box_off[0] != 0) return (int)hipErrorInvalidValue;
  for (int b = 0; b < batch; ++b) {
    const int d = box_off[b + 1] - box_off[b];
    if (d < 0 || d > kMaxBoxes) return (int)hipErrorInvalidValue;
  }
  for (int b = 0; b <= kMaxFrames; ++b) a.box_off[b] = box_off[b <= batch ? b : batch];
  const int n_boxes = box_off[batch];
  for (int j = 0; j < 12; ++j) a.m[j] = m[j];
  a.bin_w = bin_w;
  a.min_depth = min_depth;
  a.window = window;
  if (n_boxes == 0) return 0;
  if (table == nullptr || hist == nullptr || out == nullptr || (max_n > 0 && data == nullptr))
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)table & 15) != 0 || ((uintptr_t)hist & 15) != 0 || ((uintptr_t)out & 7) != 0 ||
      ((uintptr_t)frame_off & 7) != 0 || ((uintptr_t)frame_n & 3) != 0)
    return (int)hipErrorInvalidValue;
  if (int e = zero_i32_async(hist, n_boxes * kBins, stream)) return e;
  const dim3 grid((max_n + kBlock - 1) / kBlock, batch);
  if (max_n > 0) {
    range2d_points_kernel<1><<<grid, kBlock, 0, stream>>>((const uint8_t*)data, data_bytes, frame_off, frame_n, a,
                                                          (const float4*)table, hist, (int*)out);
    if (int e = (int)hipGetLastError()) return e;
  }
  range2d_select_kernel<<<(n_boxes + kBlock / 64 - 1) / (kBlock / 64), kBlock, 0, stream>>>(hist, n_boxes, pct,
                                                                                         min_points, (int*)out);
  if (int e = (int)hipGetLastError()) return e;
  if (max_n > 0)
    range2d_points_kernel<2><<<grid, kBlock, 0, stream>>>((const uint8_t*)data, data_bytes, frame_off, frame_n, a,
                                                          (const float4*)table, hist, (int*)out);
  TCA_LAUNCH_CHECK();
}

TCA_API int tca_range2d_bins() { return kBins; }
