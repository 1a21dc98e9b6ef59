// K33 — the cloud as a ray-cast occupancy grid: per cell of a bird's-eye grid 100 (occupied), 0 (free) or -1
// (unknown), from the obstacle and ground records K30 left on the device.
//
// Batched over B <= 64 clouds that share one field layout.  The launch runs behind tca_ground_split(want = 3) on
// the same stream and reads its output slab in place (tca_cloud_load.h): slot b starts at frame_off[b] and holds
// frame_n[b] records, the first counts[b][0] of them obstacles, the last counts[b][1] ground.  A record's class is
// its position: no class byte is read.  ops/occupancy_grid.py has the definition: float32, every operation rounded
// on its own.  The grid is W x H cells, row-major, cell = iy * W + ix; directions are S sectors (the laser scan's
// pseudo-angle against a host-built table of S + 1 non-decreasing edges, K29).
//
//   reset    the cell words uint32[B][stride] = 0, near uint32[B][S] = 0xFFFFFFFF, far uint32[B][S] = 0.
//   points   blockIdx.y = cloud; one index space over the slot's obstacle records, then its ground records.  A
//            workgroup keeps the S + 1 edges and its own near / far bins in LDS ((3 S + 1) * 4 bytes, 48 KiB at
//            S = 4096), walks 256-record blocks with a stride of gridDim.x blocks, finds each record's sector by
//            binary search in LDS (13 steps at most) and takes near with LDS atomicMin (obstacles) and far with LDS
//            atomicMax (both classes) of r's bits: positive floats order as their bits.  After one __syncthreads()
//            only the touched bins go to global, one atomic each.  A cell word holds the obstacle count in its low
//            31 bits (a launch has fewer than 2^28 records) and the ground flag in bit 31; a sensor's records
//            arrive in azimuth order, so a wave's lanes fall into runs of equal cells (wave_run, tca_cluster.h) and
//            one atomicAdd of the run's length, or one atomicOr, per run goes to global.  privatise = 0 sends every
//            key to global, aggregate = 0 every record's cell: the same bytes, for measurements.
//   cells    blockIdx.y = cloud; a thread owns four consecutive cells of the flat plane: one 16-byte load of their
//            words, per cell the value rule, one 32-bit store of the four int8 (a plane starts 16-byte aligned in
//            the output; a tail of fewer than four cells is written bytewise).  Occupied cells and cells with a
//            ground return are decided by their word alone; the others need the centre's r_c and, outside
//            clear_radius, its sector (edges in LDS) and min(near, far) of it: from global (8 S bytes per cloud,
//            read by every workgroup of the cloud and cached), or with stage_keys = 1 from LDS.
//
// The reset belongs to the launch and only integer atomics are used, so no output depends on the order blocks run
// in and a relaunch or a graph replay gives the same bytes.  Nothing is allocated and no hipMemset is used.
#include "tca_cloud_load.h"
#include "tca_cluster.h"
#include "tca_common.h"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

using namespace tca;

namespace {

constexpr int kBlock = 256;
constexpr int kMaxFrames = 64;
constexpr int kMaxSectors = 4096;
constexpr int kMaxSide = 2048;
constexpr int kMaxCells = 1 << 22;
constexpr int kMaxPlane = 1 << 24;
constexpr uint32_t kNoKey = 0xFFFFFFFFu;
constexpr uint32_t kGroundBit = 0x80000000u;
constexpr float kFltMax = 3.402823466e+38f;

struct GridArgs {
  int step;
  int off[4];  // x, y, z, -1
  int fast;    // tca_cloud_load.h
  int S, W, H;
  int stride;  // cells from one cloud's plane to the next: a multiple of 16
  int max_n, min_pts;
  float x0, y0, c32, clear;
};

__global__ void __launch_bounds__(kBlock) grid_reset_kernel(uint32_t* __restrict__ cells, int n_cells,
                                                            uint32_t* __restrict__ keys, int batch, int S) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n_cells) cells[i] = 0u;
  if (i < 2 * batch * S) keys[i] = (i / S) & 1 ? 0u : kNoKey;  // [B][2][S]: near, far
}

// The sector of direction (x, y) by the definition's pseudo-angle against the S + 1 edges in `tab`, -1 without one.
__device__ __forceinline__ int sector_of(float x, float y, const float* tab, int S) {
  const float s = fabsf(x) + fabsf(y);
  if (!(s != 0.f && s <= kFltMax)) return -1;  // zero, infinite or NaN
  const float q = copysignf(1.f - x / s, y);
  if (!(q >= tab[0] && q <= tab[S])) return -1;
  int lo = 0, hi = S + 1;  // the number of edges <= q: searchsorted(table, q, "right")
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tab[mid] <= q) lo = mid + 1; else hi = mid;
  }
  // q >= t0: lo >= 1; q == tS: sector S - 1; the clamp only matters for a table that is not sorted
  return min(max(lo - 1, 0), S - 1);
}

// The point's cell by ops/cluster.py's rule with z_range = +-512, -1 where it is not valid (a NaN compares false).
__device__ __forceinline__ int point_cell(float x, float y, float z, const GridArgs& a) {
  if (!(fabsf(x) <= 512.f && fabsf(y) <= 512.f && fabsf(z) <= 512.f)) return -1;
  const float dx = (x - a.x0) / a.c32, dy = (y - a.y0) / a.c32;
  if (!(dx >= 0.f && dx < (float)a.W && dy >= 0.f && dy < (float)a.H)) return -1;
  return min((int)dy, a.H - 1) * a.W + min((int)dx, a.W - 1);  // (the clamps change nothing)
}

// ---------------------------------------------------------------------------------- points
template <bool kLds, bool kAggregate>
__global__ void __launch_bounds__(kBlock) grid_points_kernel(
    const uint8_t* __restrict__ data, long data_bytes, const long* __restrict__ frame_off,
    const int* __restrict__ frame_n, const int* __restrict__ counts, const float* __restrict__ table, GridArgs a,
    uint32_t* __restrict__ cells, uint32_t* __restrict__ keys) {
  extern __shared__ uint32_t lds[];
  float* tab = reinterpret_cast<float*>(lds);  // S + 1 edges
  uint32_t* s_near = lds + a.S + 1;            // S keys each (kLds)
  uint32_t* s_far = s_near + a.S;

  const int b = blockIdx.y;
  const int n = min(max(frame_n[b], 0), a.max_n);
  const int n_obs = min(max(counts[2 * b], 0), n), n_gnd = min(max(counts[2 * b + 1], 0), n - n_obs);
  const int n_pts = n_obs + n_gnd;
  const int n_blocks = (n_pts + kBlock - 1) / kBlock;
  if ((int)blockIdx.x >= n_blocks) return;  // the whole workgroup: nothing of this cloud is its own
  const long foff = frame_off[b];
  const int path = cloud_frame_path(a.fast, foff);
  uint32_t* plane = cells + (long)b * a.stride;
  uint32_t* g_near = keys + (long)b * 2 * a.S;
  uint32_t* g_far = g_near + a.S;

  for (int i = threadIdx.x; i <= a.S; i += kBlock) tab[i] = table[i];
  if (kLds)
    for (int i = threadIdx.x; i < a.S; i += kBlock) { s_near[i] = kNoKey; s_far[i] = 0u; }
  __syncthreads();
  uint32_t* near = kLds ? s_near : g_near;
  uint32_t* far = kLds ? s_far : g_far;

  for (int blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {  // (the same trips for every lane)
    const int i = blk * kBlock + threadIdx.x;
    const bool gnd = i >= n_obs;
    const long rec = gnd ? (long)(n - n_gnd) + (i - n_obs) : (long)i;  // the ground region ends the slot
    const long at = foff + rec * a.step;
    int run_key = -1;  // cell * 2 + class: a run is of one cell and one class
    // a record outside the buffer is not read
    if (i < n_pts && foff >= 0 && foff <= data_bytes && at + a.step <= data_bytes) {
      uint32_t raw[4] = {0u, 0u, 0u, 0u};
      cloud_load_fields(data + at, a.off, path, raw);
      const float x = __uint_as_float(raw[0]), y = __uint_as_float(raw[1]), z = __uint_as_float(raw[2]);
      const int cell = point_cell(x, y, z, a);
      if (cell >= 0) run_key = 2 * cell + (gnd ? 1 : 0);
      const int sec = sector_of(x, y, tab, a.S);
      const float r = sqrtf(x * x + y * y);
      if (sec >= 0 && r <= kFltMax) {
        const uint32_t key = __float_as_uint(r);  // r >= 0
        if (!gnd) atomicMin(near + sec, key);
        atomicMax(far + sec, key);
      }
    }
    if (kAggregate) {
      const Run run = wave_run(run_key);
      if (run.head) {
        if (run_key & 1) atomicOr(plane + (run_key >> 1), kGroundBit);
        else atomicAdd(plane + (run_key >> 1), (uint32_t)run.len);
      }
    } else if (run_key >= 0) {
      if (run_key & 1) atomicOr(plane + (run_key >> 1), kGroundBit);
      else atomicAdd(plane + (run_key >> 1), 1u);
    }
  }

  if (kLds) {
    __syncthreads();
    for (int i = threadIdx.x; i < a.S; i += kBlock) {
      const uint32_t lo = s_near[i], hi = s_far[i];
      if (lo != kNoKey) atomicMin(g_near + i, lo);
      if (hi != 0u) atomicMax(g_far + i, hi);
    }
  }
}

// ----------------------------------------------------------------------------------- cells
__device__ __forceinline__ int cell_value(uint32_t word, int ix, int iy, const GridArgs& a, const float* tab,
                                          const uint32_t* near, const uint32_t* far) {
  if ((word & ~kGroundBit) >= (uint32_t)a.min_pts) return 100;
  if (word & kGroundBit) return 0;
  const float cx = a.x0 + ((float)ix + 0.5f) * a.c32, cy = a.y0 + ((float)iy + 0.5f) * a.c32;
  const float r = sqrtf(cx * cx + cy * cy);
  if (r < a.clear) return 0;
  const int sec = sector_of(cx, cy, tab, a.S);
  if (sec < 0) return -1;
  return __float_as_uint(r) < min(near[sec], far[sec]) ? 0 : -1;
}

template <bool kStage>
__global__ void __launch_bounds__(kBlock) grid_cells_kernel(const float* __restrict__ table, GridArgs a,
                                                            const uint32_t* __restrict__ cells,
                                                            const uint32_t* __restrict__ keys,
                                                            int8_t* __restrict__ out) {
  extern __shared__ uint32_t lds[];
  float* tab = reinterpret_cast<float*>(lds);  // S + 1 edges
  const int b = blockIdx.y;
  const uint32_t* near = keys + (long)b * 2 * a.S;
  const uint32_t* far = near + a.S;
  for (int i = threadIdx.x; i <= a.S; i += kBlock) tab[i] = table[i];
  if (kStage) {
    uint32_t* s_keys = lds + a.S + 1;  // near, then far, as in global
    for (int i = threadIdx.x; i < 2 * a.S; i += kBlock) s_keys[i] = near[i];
    near = s_keys;
    far = s_keys + a.S;
  }
  __syncthreads();

  const int n_cells = a.W * a.H;
  const int n_chunks = (n_cells + 4 * kBlock - 1) / (4 * kBlock);
  const uint32_t* plane = cells + (long)b * a.stride;
  int8_t* mine = out + (long)b * a.stride;
  for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    const int c0 = (chunk * kBlock + threadIdx.x) * 4;
    if (c0 >= n_cells) continue;
    const int cnt = min(4, n_cells - c0);
    // stride is a multiple of 16 cells and c0 of 4: the four words are inside the cloud's plane and 16-byte aligned
    const uint4 w4 = *reinterpret_cast<const uint4*>(plane + c0);
    const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
    int ix = c0 % a.W, iy = c0 / a.W;
    uint32_t packed = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < cnt) packed |= ((uint32_t)cell_value(w[j], ix, iy, a, tab, near, far) & 0xFFu) << (8 * j);
      if (++ix == a.W) { ix = 0; ++iy; }
    }
    if (cnt == 4) {
      *reinterpret_cast<uint32_t*>(mine + c0) = packed;
    } else {
      for (int j = 0; j < cnt; ++j) mine[c0 + j] = (int8_t)(packed >> (8 * j));
    }
  }
}

}  // namespace

// data: K30's output slab, data_bytes of it (no record outside is read); frame_off long[B] (bytes), frame_n int[B] (the
// staged records of every slot) and counts int[B][2] (obstacles, ground: what K30 wrote): device; max_n: the largest
// frame_n the host knows (sizes the grid; the kernels clamp to it); offsets of x, y, z in a record of FLOAT32 fields.
// table: device float[sectors + 1], non-decreasing.  x_min, y_min, cell, clear_radius: the float32 values of
// ops/occupancy_grid.py; W x H cells; a cell is occupied from min_points obstacle points.  privatise: 1, the sector
// keys in LDS; aggregate: 1, one atomic per run of equal cells of a wave; stage_keys: 1, the cell pass reads near / far
// from LDS (0 / 0 / 1: measurements).  Workspace, reset here on the stream: cells uint32[B][stride] with stride =
// ceil(W * H / 16) * 16 (16-byte aligned), keys uint32[B][2][sectors].  out: int8, cloud b's W * H cells at
// out + b * stride (16-byte aligned); nothing past (B - 1) * stride + W * H is written.  A workspace or an output
// shorter than that is refused.
TCA_API int tca_occupancy_grid(const void* data, long data_bytes, const long* frame_off, const int* frame_n,
                               const int* counts, int batch, int max_n, int point_step, int off_x, int off_y,
                               int off_z, const float* table, int sectors, float x_min, float y_min, float cell, int W,
                               int H, int min_points, float clear_radius, int privatise, int aggregate,
                               int stage_keys, void* cells, long cells_bytes, void* keys, long keys_bytes, void* out,
                               long out_bytes, hipStream_t stream) {
  if (batch < 1 || batch > kMaxFrames || max_n < 0 || point_step <= 0 || data_bytes < 0 ||
      data_bytes >= 0x80000000L)
    return (int)hipErrorInvalidValue;
  if (sectors < 1 || sectors > kMaxSectors || W < 1 || W > kMaxSide || H < 1 || H > kMaxSide ||
      (long)W * H > kMaxCells || min_points < 1)
    return (int)hipErrorInvalidValue;
  if ((privatise != 0 && privatise != 1) || (aggregate != 0 && aggregate != 1) || (stage_keys != 0 && stage_keys != 1))
    return (int)hipErrorInvalidValue;
  if (!std::isfinite(cell) || !(cell > 0.f) || !std::isfinite(x_min) || !std::isfinite(y_min) ||
      !std::isfinite(clear_radius) || !(clear_radius >= 0.f))
    return (int)hipErrorInvalidValue;
  const long stride = ((long)W * H + 15) / 16 * 16;
  if ((long)batch * stride > kMaxPlane) return (int)hipErrorInvalidValue;
  if (cells_bytes < 4 * batch * stride || keys_bytes < 8L * batch * sectors ||
      out_bytes < (batch - 1) * stride + (long)W * H)
    return (int)hipErrorInvalidValue;
  if (table == nullptr || frame_off == nullptr || frame_n == nullptr || counts == nullptr || cells == nullptr ||
      keys == nullptr || out == nullptr || (max_n > 0 && data == nullptr))
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)cells & 15) != 0 || ((uintptr_t)out & 15) != 0 || ((uintptr_t)keys & 3) != 0 ||
      ((uintptr_t)table & 3) != 0 || ((uintptr_t)counts & 3) != 0 || ((uintptr_t)frame_off & 7) != 0 ||
      ((uintptr_t)frame_n & 3) != 0)
    return (int)hipErrorInvalidValue;
  GridArgs a;
  a.step = point_step;
  a.off[0] = off_x; a.off[1] = off_y; a.off[2] = off_z; a.off[3] = -1;
  a.fast = cloud_fast_path(data, point_step, a.off, true);
  if (a.fast < 0) return (int)hipErrorInvalidValue;
  a.S = sectors; a.W = W; a.H = H; a.stride = (int)stride; a.max_n = max_n; a.min_pts = min_points;
  a.x0 = x_min; a.y0 = y_min; a.c32 = cell; a.clear = clear_radius;

  const int n_words = batch * (int)stride;  // <= 2^24
  const int n_reset = std::max(n_words, 2 * batch * sectors);
  grid_reset_kernel<<<(unsigned)((n_reset + kBlock - 1) / kBlock), kBlock, 0, stream>>>((uint32_t*)cells, n_words,
                                                                                        (uint32_t*)keys, batch, sectors);
  if (int e = (int)hipGetLastError()) return e;
  if (max_n > 0) {
    const int blocks = (max_n + kBlock - 1) / kBlock;
    // blocks per workgroup: the LDS fill and flush (5 S / 256 passes) stay a fraction of the walk, as in K29
    const int k = std::min(32, std::max(4, sectors / 64));
    const dim3 grid((blocks + k - 1) / k, batch);
    const size_t lds = (size_t)(3 * sectors + 1) * sizeof(uint32_t);
    const uint8_t* in = (const uint8_t*)data;
    uint32_t* cw = (uint32_t*)cells;
    uint32_t* kw = (uint32_t*)keys;
    if (privatise && aggregate)
      grid_points_kernel<true, true><<<grid, kBlock, lds, stream>>>(in, data_bytes, frame_off, frame_n, counts, table,
                                                                    a, cw, kw);
    else if (privatise)
      grid_points_kernel<true, false><<<grid, kBlock, lds, stream>>>(in, data_bytes, frame_off, frame_n, counts,
                                                                     table, a, cw, kw);
    else if (aggregate)
      grid_points_kernel<false, true><<<grid, kBlock, lds, stream>>>(in, data_bytes, frame_off, frame_n, counts,
                                                                     table, a, cw, kw);
    else
      grid_points_kernel<false, false><<<grid, kBlock, lds, stream>>>(in, data_bytes, frame_off, frame_n, counts,
                                                                      table, a, cw, kw);
    if (int e = (int)hipGetLastError()) return e;
  }
  const int n_chunks = (W * H + 4 * kBlock - 1) / (4 * kBlock);
  // chunks of 1024 cells per workgroup: the edge table's fill stays a fraction of the walk
  const int k = std::min(32, std::max(1, sectors / 128));
  const dim3 cgrid((n_chunks + k - 1) / k, batch);
  if (stage_keys)
    grid_cells_kernel<true><<<cgrid, kBlock, (size_t)(3 * sectors + 1) * sizeof(uint32_t), stream>>>(
        table, a, (const uint32_t*)cells, (const uint32_t*)keys, (int8_t*)out);
  else
    grid_cells_kernel<false><<<cgrid, kBlock, (size_t)(sectors + 1) * sizeof(uint32_t), stream>>>(
        table, a, (const uint32_t*)cells, (const uint32_t*)keys, (int8_t*)out);
  TCA_LAUNCH_CHECK();
}
