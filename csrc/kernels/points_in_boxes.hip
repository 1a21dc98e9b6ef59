// K22 — points in boxes: which detection owns which LiDAR point (OpenPCDet ships the
// primitive as roiaware_pool3d's points_in_boxes_gpu; here it labels the published cloud
// and counts the points of ground-truth boxes for the evaluator).
//
// Batched over B clouds that share one field layout.  Raw PointCloud2 bytes are read in
// place as in K6 (per-frame byte offset + point count in device arrays); the boxes are
// ragged (box_off[B + 1]) rows of a table the host prepares:
//   row k = (cx, cy, cz, hx, hy, hz, cos yaw, sin yaw), all NaN for a box that contains
//   nothing (a non-finite entry, a dimension <= 0), so no transcendental runs here.
// One lane per point, blocks of 256.  The frame's table goes through LDS in chunks of
// kChunk boxes (any K works); every lane reads the same row at a time (an LDS broadcast).
// Per chunk each wave adds its ballot population to an LDS integer per box, and the block
// issues one global integer atomicAdd per box with a non-zero count: integer sums, so the
// counts do not depend on the order the blocks finish in.
//
// The arithmetic is the float32 definition of ops/points_in_boxes.py, every operation
// rounded on its own: contraction to FMA is switched off for this file.
#include "tca_common.h"

#pragma clang fp contract(off)

using namespace tca;

namespace {

constexpr int kBlock = 256;
constexpr int kChunk = 128;     // boxes per LDS stage
constexpr int kRecord = 28;     // bytes of an output record: x, y, z, intensity, label, instance, score

struct PibLayout {
  int step;
  int off[4];  // byte offset of x, y, z, intensity in a record; intensity -1: the cloud has none
  // 2: x, y, z, intensity are the 16 B at 0 / 4 / 8 / 12, step % 16 == 0 and the base pointer is 16-B aligned
  //    (one 16-B load per point); 1: offsets, step and base pointer are 4-B aligned (dword loads); 0: byte loads.
  // The frame's byte offset must be as aligned, checked per block.
  int fast;
};

__device__ __forceinline__ uint32_t load_u32_bytes(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

__global__ void __launch_bounds__(kBlock) points_in_boxes_kernel(
    const uint8_t* __restrict__ data, const long* __restrict__ frame_off, const int* __restrict__ frame_n,
    PibLayout lay, const int* __restrict__ box_off, const float* __restrict__ table, const float* __restrict__ score,
    const int* __restrict__ label, const int* __restrict__ pt_off, int* __restrict__ owner, int* __restrict__ count,
    uint32_t* __restrict__ record) {
  __shared__ float s_tab[kChunk * 8];
  __shared__ float s_score[kChunk];
  __shared__ int s_cnt[kChunk];
  const int b = blockIdx.y;
  const int n = frame_n[b];
  if ((long)blockIdx.x * kBlock >= n) return;  // block-uniform: before any barrier
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < n;
  const long foff = frame_off[b];
  const int fast = (lay.fast == 2 && (foff & 15) == 0) ? 2 : (lay.fast >= 1 && (foff & 3) == 0) ? 1 : 0;

  uint32_t raw[4] = {0u, 0u, 0u, 0u};
  if (live) {
    const uint8_t* rec = data + foff + (long)i * lay.step;
    if (fast == 2) {
      const uint4 q = *reinterpret_cast<const uint4*>(rec);
      raw[0] = q.x; raw[1] = q.y; raw[2] = q.z; raw[3] = q.w;
    } else if (fast == 1) {
#pragma unroll
      for (int f = 0; f < 4; ++f)
        if (lay.off[f] >= 0) raw[f] = *reinterpret_cast<const uint32_t*>(rec + lay.off[f]);
    } else {
#pragma unroll
      for (int f = 0; f < 4; ++f)
        if (lay.off[f] >= 0) raw[f] = load_u32_bytes(rec + lay.off[f]);
    }
  }
  const float x = __uint_as_float(raw[0]), y = __uint_as_float(raw[1]), z = __uint_as_float(raw[2]);

  const int k0 = box_off[b], k1 = box_off[b + 1];
  int best = -1;
  float best_score = 0.f;
  for (int c0 = k0; c0 < k1; c0 += kChunk) {
    const int nb = min(kChunk, k1 - c0);
    __syncthreads();  // the previous chunk's counts are flushed
    for (int j = threadIdx.x; j < nb * 8; j += kBlock) s_tab[j] = table[(long)c0 * 8 + j];
    if (threadIdx.x < nb) {
      s_score[threadIdx.x] = score[c0 + threadIdx.x];
      s_cnt[threadIdx.x] = 0;
    }
    __syncthreads();
    for (int j = 0; j < nb; ++j) {
      const float* t = s_tab + j * 8;
      const float ex = x - t[0], ey = y - t[1], ez = z - t[2];
      const float c = t[6], s = t[7];
      const float lx = (ex * c) + (ey * s);
      const float ly = (ey * c) - (ex * s);
      // closed faces; a NaN anywhere (point or box row) compares false
      const bool in = live && fabsf(lx) <= t[3] && fabsf(ly) <= t[4] && fabsf(ez) <= t[5];
      const unsigned long long m = __ballot(in);
      if (m != 0ull && (threadIdx.x & 63) == 0) atomicAdd(&s_cnt[j], __popcll(m));
      if (in) {
        const float sc = s_score[j];
        if (best < 0 || sc > best_score) {  // ascending k: a tie keeps the lower index
          best = c0 - k0 + j;
          best_score = sc;
        }
      }
    }
    __syncthreads();
    if (threadIdx.x < nb && s_cnt[threadIdx.x] != 0) atomicAdd(&count[c0 + threadIdx.x], s_cnt[threadIdx.x]);
  }
  if (!live) return;
  const long o = (long)pt_off[b] + i;
  owner[o] = best;
  if (record != nullptr) {
    uint32_t* r = record + o * (kRecord / 4);
    r[0] = raw[0];
    r[1] = raw[1];
    r[2] = raw[2];
    r[3] = raw[3];
    r[4] = best >= 0 ? (uint32_t)label[k0 + best] : 0u;
    r[5] = (uint32_t)best;
    r[6] = best >= 0 ? __float_as_uint(best_score) : 0u;
  }
}

}  // namespace

// data: device bytes; frame_off long[B] (bytes) / frame_n int[B]: device; max_n: the largest frame_n (host, sizes the
// grid); offsets of x, y, z, intensity (-1: none) in a record of FLOAT32 fields.  box_off int[B + 1], table
// float[K, 8], score float[K], label int[K], pt_off int[B + 1]: device.  owner int[pt_off[B]], count int[K] (zeroed
// here, on the stream), record: 28 B per point or null.
TCA_API int tca_points_in_boxes(const void* data, const long* frame_off, const int* frame_n, int batch, int max_n,
                                int point_step, int off_x, int off_y, int off_z, int off_i, const int* box_off,
                                const float* table, const float* score, const int* label, int n_boxes,
                                const int* pt_off, int* owner, int* count, void* record, hipStream_t stream) {
  if (batch < 0 || max_n < 0 || n_boxes < 0 || point_step <= 0) return (int)hipErrorInvalidValue;
  PibLayout lay;
  lay.step = point_step;
  lay.off[0] = off_x; lay.off[1] = off_y; lay.off[2] = off_z; lay.off[3] = off_i;
  bool dword = (point_step & 3) == 0 && ((uintptr_t)data & 3) == 0;
  for (int f = 0; f < 4; ++f) {
    const int o = lay.off[f];
    if (f == 3 && o == -1) continue;
    if (o < 0 || o + 4 > point_step) return (int)hipErrorInvalidValue;
    dword = dword && (o & 3) == 0;
  }
  lay.fast = !dword ? 0
             : (off_x == 0 && off_y == 4 && off_z == 8 && off_i == 12 && (point_step & 15) == 0 &&
                ((uintptr_t)data & 15) == 0) ? 2 : 1;
  if (((uintptr_t)owner & 3) != 0 || ((uintptr_t)record & 3) != 0) return (int)hipErrorInvalidValue;
  if (n_boxes > 0) {
    const int e = zero_i32_async(count, n_boxes, stream);
    if (e) return e;
  }
  if (batch == 0 || max_n == 0) return 0;
  dim3 grid((max_n + kBlock - 1) / kBlock, batch);
  points_in_boxes_kernel<<<grid, kBlock, 0, stream>>>((const uint8_t*)data, frame_off, frame_n, lay, box_off, table,
                                                      score, label, pt_off, owner, count, (uint32_t*)record);
  TCA_LAUNCH_CHECK();
}

TCA_API int tca_points_in_boxes_chunk() { return kChunk; }
