// K29 — the cloud as a 2D LaserScan: per angular bin around the sensor's z axis, the range of the
// nearest return in a height band.
//
// Batched over B <= 64 clouds that share one field layout.  Raw PointCloud2 bytes are read in
// place (tca_cloud_load.h: 16-byte record, dwords or bytes, chosen from the alignment of the
// base pointer and of each frame's offset).  The bins' edges come as a table of n + 1
// non-decreasing pseudo-angles, built on the host (ops/laser_scan.py).
//
//   reset    the key plane uint32[B][n] is set to 0xFFFFFFFF.
//   points   blockIdx.y = cloud.  There are 120k points to a cloud and a few hundred to 4096 bins:
//            one global atomicMin per point would put hundreds of lanes on a handful of addresses.
//            So a workgroup keeps its cloud's n bins (and the n + 1 edges) in LDS, walks
//            256-point blocks of the cloud with a stride of gridDim.x blocks, takes the minima
//            with LDS integer atomicMin and, after one __syncthreads(), flushes only the bins it
//            touched with one global atomicMin each.  A point's bin is searchsorted(table, q,
//            "right") - 1 by binary search in LDS: 13 steps at most.
//   convert  the plane becomes float[B][n]; an untouched bin gets the empty value.
//
// Points per workgroup.  Per workgroup the LDS fill (2n + 1 dwords) and the flush (n dwords) cost
// about 3n / 256 passes of the block; a 256-point block costs one record load and up to 13
// dependent LDS reads.  With k = clamp(n / 128, 4, 32) blocks per workgroup the fixed part stays
// below a quarter of the per-point part (n = 4096: 48 passes against 32 blocks of ~14 steps), and
// a 120k-point cloud still spreads over 15 (n = 4096) to 118 (n <= 512) workgroups.  The grid is
// ceil(ceil(max_n / 256) / k) x B; a workgroup whose cloud has no block for it leaves at once.
// LDS per workgroup is (2n + 1) * 4 bytes, 32 KiB at most: five workgroups fit a CU's 160 KiB.
//
// The reset belongs to the launch: a relaunch or a graph replay gives the same bytes.  Only
// integer atomics are used (positive floats order as their bits), so no output depends on the
// order blocks run in.  The arithmetic is the float32 definition of ops/laser_scan.py, every
// operation rounded on its own: contraction to FMA is switched off for this file, division and
// square root are IEEE.
#include "tca_cloud_load.h"
#include "tca_common.h"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

using namespace tca;

namespace {

constexpr int kBlock = 256;
constexpr int kMaxFrames = 64;
constexpr int kMaxBins = 4096;
constexpr uint32_t kEmpty = 0xFFFFFFFFu;

struct ScanArgs {
  int step;
  int off[4];  // x, y, z, -1
  int fast;    // tca_cloud_load.h
  int n;       // bins
  float h0, h1, r0, r1;
};

__global__ void __launch_bounds__(kBlock) scan_reset_kernel(uint32_t* __restrict__ plane, int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) plane[i] = kEmpty;
}

// kLds: the workgroup's own bins in LDS (the kernel that ships); without: every valid point does a
// global atomicMin (kept to measure what the LDS bins buy).
template <bool kLds>
__global__ void __launch_bounds__(kBlock) scan_points_kernel(
    const uint8_t* __restrict__ data, long data_bytes, const long* __restrict__ frame_off,
    const int* __restrict__ frame_n, const float* __restrict__ table, ScanArgs a, uint32_t* __restrict__ plane) {
  extern __shared__ uint32_t lds[];
  float* tab = reinterpret_cast<float*>(lds);  // n + 1 edges
  uint32_t* bins = lds + a.n + 1;              // n keys (kLds)

  const int b = blockIdx.y;
  const int n_pts = frame_n[b];
  const int n_blocks = (n_pts + kBlock - 1) / kBlock;
  if ((int)blockIdx.x >= n_blocks) return;  // the whole workgroup: nothing of this cloud is its own
  const long foff = frame_off[b];
  const int path = cloud_frame_path(a.fast, foff);
  uint32_t* row = plane + (long)b * a.n;

  for (int i = threadIdx.x; i <= a.n; i += kBlock) tab[i] = table[i];
  if (kLds)
    for (int i = threadIdx.x; i < a.n; i += kBlock) bins[i] = kEmpty;
  __syncthreads();
  const float t0 = tab[0], tn = tab[a.n];

  for (int blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const long i = (long)blk * kBlock + threadIdx.x;
    const long at = foff + i * a.step;
    // a record outside the buffer is not read
    if (!(i < n_pts && foff >= 0 && foff <= data_bytes && at + a.step <= data_bytes)) continue;

    uint32_t raw[4] = {0u, 0u, 0u, 0u};
    cloud_load_fields(data + at, a.off, path, raw);
    const float x = __uint_as_float(raw[0]), y = __uint_as_float(raw[1]), z = __uint_as_float(raw[2]);

    // a NaN compares false
    if (!(z >= a.h0 && z <= a.h1)) continue;
    const float r = sqrtf(x * x + y * y);
    if (!(r >= a.r0 && r <= a.r1)) continue;
    const float s = fabsf(x) + fabsf(y);
    if (!(s != 0.f && s <= 3.402823466e+38f)) continue;  // zero, infinite or NaN
    const float q = copysignf(1.f - x / s, y);
    if (!(q >= t0 && q <= tn)) continue;

    int lo = 0, hi = a.n + 1;  // the number of edges <= q: searchsorted(table, q, "right")
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (tab[mid] <= q) lo = mid + 1; else hi = mid;
    }
    // q >= t0: lo >= 1; q == tn: bin n - 1; the clamp only matters for a table that is not sorted
    const int bin = min(max(lo - 1, 0), a.n - 1);
    const uint32_t key = __float_as_uint(r);     // r >= range_min >= 0
    if (kLds) atomicMin(bins + bin, key);
    else atomicMin(row + bin, key);
  }

  if (kLds) {
    __syncthreads();
    for (int i = threadIdx.x; i < a.n; i += kBlock) {
      const uint32_t k = bins[i];
      if (k != kEmpty) atomicMin(row + i, k);
    }
  }
}

__global__ void __launch_bounds__(kBlock) scan_convert_kernel(const uint32_t* __restrict__ plane, int n,
                                                              uint32_t empty_bits, uint32_t* __restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t k = plane[i];
  out[i] = k == kEmpty ? empty_bits : k;
}

}  // namespace

// data: device bytes, data_bytes of them (no record outside is read); frame_off long[B] (bytes) / frame_n int[B]:
// device; max_n: the largest frame_n (host, sizes the grid); offsets of x, y, z in a record of FLOAT32 fields.
// table: device float[n_bins + 1], non-decreasing.  min_height <= z <= max_height and range_min <= r <= range_max
// keep a point.  empty_bits: the float bits an untouched bin gets.  privatise: 1, the workgroup's bins in LDS; 0,
// global atomics only (measurements).  plane: B * n_bins uint32 of workspace, reset here on the stream.  out:
// float[B][n_bins].
TCA_API int tca_laser_scan(const void* data, long data_bytes, const long* frame_off, const int* frame_n, int batch,
                           int max_n, int point_step, int off_x, int off_y, int off_z, const float* table, int n_bins,
                           float min_height, float max_height, float range_min, float range_max,
                           unsigned empty_bits, int privatise, void* plane, void* out, hipStream_t stream) {
  if (batch < 1 || batch > kMaxFrames || max_n < 0 || point_step <= 0 || data_bytes < 0 ||
      data_bytes >= 0x80000000L)
    return (int)hipErrorInvalidValue;
  if (n_bins < 1 || n_bins > kMaxBins || (privatise != 0 && privatise != 1)) return (int)hipErrorInvalidValue;
  // the heights may be infinite, nothing may be NaN
  if (std::isnan(min_height) || std::isnan(max_height) || min_height > max_height || !std::isfinite(range_min) ||
      !std::isfinite(range_max) || !(range_min >= 0.f) || !(range_min < range_max))
    return (int)hipErrorInvalidValue;
  if (table == nullptr || frame_off == nullptr || frame_n == nullptr || plane == nullptr || out == nullptr ||
      (max_n > 0 && data == nullptr))
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)plane & 3) != 0 || ((uintptr_t)out & 3) != 0 || ((uintptr_t)table & 3) != 0 ||
      ((uintptr_t)frame_off & 7) != 0 || ((uintptr_t)frame_n & 3) != 0)
    return (int)hipErrorInvalidValue;
  ScanArgs a;
  a.step = point_step;
  a.off[0] = off_x; a.off[1] = off_y; a.off[2] = off_z; a.off[3] = -1;
  a.fast = cloud_fast_path(data, point_step, a.off, true);
  if (a.fast < 0) return (int)hipErrorInvalidValue;
  a.n = n_bins;
  a.h0 = min_height; a.h1 = max_height; a.r0 = range_min; a.r1 = range_max;
  const int cells = batch * n_bins;  // <= 2^18
  const unsigned cell_blocks = (unsigned)((cells + kBlock - 1) / kBlock);
  scan_reset_kernel<<<cell_blocks, kBlock, 0, stream>>>((uint32_t*)plane, cells);
  if (int e = (int)hipGetLastError()) return e;
  if (max_n > 0) {
    const int blocks = (max_n + kBlock - 1) / kBlock;
    const int k = std::min(32, std::max(4, n_bins / 128));  // blocks per workgroup (the file header)
    const dim3 grid((blocks + k - 1) / k, batch);
    const size_t lds = (size_t)(2 * n_bins + 1) * sizeof(uint32_t);
    if (privatise)
      scan_points_kernel<true><<<grid, kBlock, lds, stream>>>((const uint8_t*)data, data_bytes, frame_off, frame_n,
                                                              table, a, (uint32_t*)plane);
    else
      scan_points_kernel<false><<<grid, kBlock, lds, stream>>>((const uint8_t*)data, data_bytes, frame_off, frame_n,
                                                               table, a, (uint32_t*)plane);
    if (int e = (int)hipGetLastError()) return e;
  }
  scan_convert_kernel<<<cell_blocks, kBlock, 0, stream>>>((const uint32_t*)plane, cells, empty_bits, (uint32_t*)out);
  TCA_LAUNCH_CHECK();
}
