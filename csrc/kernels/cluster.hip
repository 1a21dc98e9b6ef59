// K31 — the obstacle clusters of a cloud: connected components of the occupied cells of a bird's-eye
// grid (8-neighbours), and per kept component its point count, integer bounds and integer sums.
//
// Batched over B <= 64 clouds that share one field layout.  Raw PointCloud2 bytes are read in place
// (tca_cloud_load.h); frame_n is read with a stride, so the launch also runs straight behind K30 on its
// output slab and its counts int32[B][2] (n_stride = 2: the obstacle records [0, n_obs) of every slot).
// ops/cluster.py has the definition: float32 per point, every operation rounded on its own, then
// integers only.  The grid is W x H cells, row-major, cell = iy * W + ix.
//
//   reset    cnt = 0, lab = NONE, every table row emptied, found = 0, err = 0.
//   count    one lane per point, blockIdx.y = cloud: the point's cell, saved to pcell (-1: not valid),
//            and one atomicAdd into cnt per run of consecutive lanes of a wave that share a cell (a
//            sensor's points arrive in azimuth order: neighbours in the payload are neighbours in space).
//   tiles    one workgroup of 256 threads per tile of 32 x 32 cells, four cells a thread.  A tile without
//            an occupied cell (cnt >= min_cell_points) leaves after reading its counts.  Otherwise the
//            tile's labels live in LDS (1024 int32 = 4 KiB, the kernel's whole LDS budget): an occupied
//            cell starts as its own tile-local index and is united with its W, NW, N and NE neighbours
//            inside the tile (the other four directions are the same pairs seen from the other end) by a
//            union-find on LDS atomicMin.  After a barrier every cell finds its root and stores the root's
//            global cell index to lab.  Row-major order inside a tile agrees with the global order, so the
//            tile-local minimum is the global minimum of the local component.
//   merge    one lane per cell; only cells on a tile's first row, first column or last column have a W, NW,
//            N or NE neighbour in another tile.  Those pairs are united by the same routine on the global
//            plane.
//   flatten  every occupied cell stores its root to lab, and every cell that is not its own root adds its
//            count to the root's: the cnt plane becomes the size plane.  Only roots are added to and only
//            other cells are read, so no cell's count is read after it changed.
//   rank     kept roots (min_points <= size <= max_points) are numbered in ascending cell order by K30's
//            three steps: ballot counts per 256-cell block, a scan launch of its own (one workgroup per
//            cloud, which also writes found, uncapped), then the assignment: the root's k, or -1, replaces
//            its size, and rows k < max_clusters get their root.
//   stats    one lane per point: k through pcell, lab and the root's cnt; label is written; for
//            0 <= k < max_clusters the point's xi, yi, zi go into row k (atomicAdd n, three atomicMin, three
//            atomicMax, three 64-bit atomicAdd).  aggregate = 1 first reduces over each wave's runs of equal
//            k with a segmented shuffle reduction (a wave's sums fit int32: 64 * 2^19) and the run's head
//            lane issues the ten atomics; aggregate = 0 issues them per point.  Both give the same bytes.
//
// The union-find.  lab[c] <= c always; lab[c] == c makes c a root.  unite(a, b) finds both roots, and hangs
// the larger under the smaller with atomicMin(&lab[hi], lo).  If the value it replaced was hi, hi was a root
// and is now linked.  Otherwise another lane linked hi first, to `old` < hi: whichever of old and lo the
// atomicMin left in lab[hi], hi stays connected to it, and the loop goes on to unite old with lo.  Labels only
// ever decrease, and every retry continues from a strictly smaller cell, so each call ends after finitely many
// steps whatever the other lanes do: no lane or workgroup waits for another's write (reads of labels that
// others may be lowering are relaxed atomic loads, never a register copy).  A chain lab[c] < c is shorter
// than the cell count, which is also the hard trip bound of every loop; a lane that would exceed it stops and
// sets err, which the host raises on.  The components, their minima, the integer counts, bounds and sums do
// not depend on the order the links were made in, so no output depends on the order blocks run in.
// Everything a launch reads it has written itself: a relaunch or a graph replay gives the same bytes.
//
// Nothing is allocated, no hipMemset is used, only integer atomics.
#include "tca_cloud_load.h"
#include "tca_cluster.h"
#include "tca_common.h"

#include <cmath>

#pragma clang fp contract(off)

using namespace tca;

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTile = 32;
constexpr int kTileCells = kTile * kTile;
constexpr int kMaxFrames = 64;
constexpr int kMaxSide = 2048;
constexpr int kMaxCells = 1 << 22;
constexpr int kMaxPlane = 1 << 24;
constexpr int kMaxClusters = 4096;
constexpr int kNone = 0x7FFFFFFF;
constexpr int kIntMin = -0x7FFFFFFF - 1;

struct ClusterArgs {
  int step;
  int off[4];  // x, y, z, -1
  int fast;    // tca_cloud_load.h
  int W, H;
  int max_n, n_stride;
  float x0, y0, c32, z0, z1;
  int min_cell, min_pts, max_pts, max_k;
};

// ------------------------------------------------------------------------------ union-find
template <int kScope>
__device__ __forceinline__ int lab_load(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, kScope);
}

// The root of c, or -1 past `bound` steps.
template <int kScope>
__device__ __forceinline__ int uf_find(const int* lab, int c, int bound) {
  for (int trip = 0; trip <= bound; ++trip) {
    const int p = lab_load<kScope>(lab + c);
    if (p == c) return c;
    c = p;
  }
  return -1;
}

// Unites the sets of a and b; false past `bound` steps.
template <int kScope>
__device__ __forceinline__ bool uf_unite(int* lab, int a, int b, int bound) {
  for (int trip = 0; trip <= bound; ++trip) {
    a = uf_find<kScope>(lab, a, bound);
    b = uf_find<kScope>(lab, b, bound);
    if (a < 0 || b < 0) return false;
    if (a == b) return true;
    const int hi = max(a, b), lo = min(a, b);
    const int old = atomicMin(lab + hi, lo);
    if (old == hi) return true;  // hi was a root and now hangs under lo
    a = old;                     // linked by another lane meanwhile: old < hi is still to be united with lo
    b = lo;
  }
  return false;
}

// ----------------------------------------------------------------------------------- reset
__global__ void __launch_bounds__(kBlock) cluster_reset_kernel(int* __restrict__ cnt, int* __restrict__ lab,
                                                               int cells, Row* __restrict__ table, int rows,
                                                               int* __restrict__ found, int batch,
                                                               int* __restrict__ err) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < cells) {
    cnt[i] = 0;
    lab[i] = kNone;
  }
  if (i < rows) {
    Row r;
    r.n = 0; r.root = -1;
    r.min_x = r.min_y = r.min_z = kNone;
    r.max_x = r.max_y = r.max_z = kIntMin;
    r.sum_x = r.sum_y = r.sum_z = r.pad = 0;
    table[i] = r;
  }
  if (i < batch) found[i] = 0;
  if (i == 0) *err = 0;
}

// ---------------------------------------------------------------------------------- points
__device__ __forceinline__ int cloud_points(const int* frame_n, int b, const ClusterArgs& a) {
  return min(max(frame_n[(long)b * a.n_stride], 0), a.max_n);
}

// Is record i of the cloud at foff inside the buffer; if so its x, y, z.
__device__ __forceinline__ bool load_point(const uint8_t* __restrict__ data, long data_bytes, long foff, long i,
                                           int n_pts, const ClusterArgs& a, int path, float* x, float* y,
                                           float* z) {
  const long at = foff + i * a.step;
  if (!(i < n_pts && foff >= 0 && foff <= data_bytes && at + a.step <= data_bytes)) return false;
  uint32_t raw[4] = {0u, 0u, 0u, 0u};
  cloud_load_fields(data + at, a.off, path, raw);
  *x = __uint_as_float(raw[0]);
  *y = __uint_as_float(raw[1]);
  *z = __uint_as_float(raw[2]);
  return true;
}

// The point's cell by the definition, -1 where it is not valid (a NaN compares false).
__device__ __forceinline__ int point_cell(float x, float y, float z, const ClusterArgs& a) {
  if (!(fabsf(x) <= 512.f && fabsf(y) <= 512.f && fabsf(z) <= 512.f && z >= a.z0 && z <= a.z1)) return -1;
  const float dx = (x - a.x0) / a.c32, dy = (y - a.y0) / a.c32;
  if (!(dx >= 0.f && dx < (float)a.W && dy >= 0.f && dy < (float)a.H)) return -1;
  return min((int)dy, a.H - 1) * a.W + min((int)dx, a.W - 1);  // (the clamps change nothing)
}

__global__ void __launch_bounds__(kBlock) cluster_count_kernel(
    const uint8_t* __restrict__ data, long data_bytes, const long* __restrict__ frame_off,
    const int* __restrict__ frame_n, ClusterArgs a, int* __restrict__ cnt, int* __restrict__ pcell) {
  const int b = blockIdx.y;
  const int n_pts = cloud_points(frame_n, b, a);
  if ((long)blockIdx.x * kBlock >= n_pts) return;  // the whole workgroup
  const long foff = frame_off[b];
  const int path = cloud_frame_path(a.fast, foff);
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  float x, y, z;
  int cell = -1;
  if (load_point(data, data_bytes, foff, i, n_pts, a, path, &x, &y, &z)) {
    cell = point_cell(x, y, z, a);
    pcell[(foff + i * a.step) / a.step] = cell;
  }
  const Run r = wave_run(cell);
  if (r.head) atomicAdd(cnt + (long)b * a.W * a.H + cell, r.len);
}

// ----------------------------------------------------------------------------------- tiles
__global__ void __launch_bounds__(kBlock) cluster_tiles_kernel(const int* __restrict__ cnt, int* __restrict__ lab,
                                                               ClusterArgs a, int* __restrict__ err) {
  __shared__ int s_lab[kTileCells];
  constexpr int kWg = __HIP_MEMORY_SCOPE_WORKGROUP;

  const int tiles_x = (a.W + kTile - 1) / kTile;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const long plane = (long)blockIdx.y * a.W * a.H;
  const int lx = threadIdx.x & 31, gx = tx * kTile + lx;
  bool occ[4];
  int any = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ly = (threadIdx.x >> 5) + 8 * j, gy = ty * kTile + ly;
    occ[j] = gx < a.W && gy < a.H && cnt[plane + (long)gy * a.W + gx] >= a.min_cell;
    s_lab[ly * kTile + lx] = occ[j] ? ly * kTile + lx : kNone;
    any |= occ[j];
  }
  if (!__syncthreads_or(any)) return;  // lab is NONE since the reset

  bool ok = true;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ly = (threadIdx.x >> 5) + 8 * j, l = ly * kTile + lx;
    if (!occ[j]) continue;
    // an occupied cell's label is below 1024 whatever is going on: NONE means not occupied
    if (lx > 0 && lab_load<kWg>(s_lab + l - 1) != kNone) ok &= uf_unite<kWg>(s_lab, l, l - 1, kTileCells);
    if (ly > 0) {
      if (lx > 0 && lab_load<kWg>(s_lab + l - kTile - 1) != kNone)
        ok &= uf_unite<kWg>(s_lab, l, l - kTile - 1, kTileCells);
      if (lab_load<kWg>(s_lab + l - kTile) != kNone) ok &= uf_unite<kWg>(s_lab, l, l - kTile, kTileCells);
      if (lx < kTile - 1 && lab_load<kWg>(s_lab + l - kTile + 1) != kNone)
        ok &= uf_unite<kWg>(s_lab, l, l - kTile + 1, kTileCells);
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ly = (threadIdx.x >> 5) + 8 * j, gy = ty * kTile + ly;
    if (!occ[j]) continue;
    const int r = uf_find<kWg>(s_lab, ly * kTile + lx, kTileCells);
    if (r < 0) { ok = false; continue; }
    lab[plane + (long)gy * a.W + gx] = (ty * kTile + (r >> 5)) * a.W + tx * kTile + (r & 31);
  }
  if (!ok) atomicOr(err, 1);
}

// ----------------------------------------------------------------------------------- merge
__global__ void __launch_bounds__(kBlock) cluster_merge_kernel(int* __restrict__ lab, ClusterArgs a,
                                                               int* __restrict__ err) {
  constexpr int kDev = __HIP_MEMORY_SCOPE_AGENT;
  const int cells = a.W * a.H;
  const int cell = blockIdx.x * kBlock + threadIdx.x;
  if (cell >= cells) return;
  const int x = cell % a.W, y = cell / a.W;
  const bool left = (x & 31) == 0, right = (x & 31) == 31, top = (y & 31) == 0;
  if (!(left || right || top)) return;  // its W, NW, N and NE neighbours are in its own tile
  int* g = lab + (long)blockIdx.y * cells;
  if (lab_load<kDev>(g + cell) == kNone) return;
  bool ok = true;
  if (x > 0 && left && lab_load<kDev>(g + cell - 1) != kNone) ok &= uf_unite<kDev>(g, cell, cell - 1, cells);
  if (y > 0) {
    if (x > 0 && (left || top) && lab_load<kDev>(g + cell - a.W - 1) != kNone)
      ok &= uf_unite<kDev>(g, cell, cell - a.W - 1, cells);
    if (top && lab_load<kDev>(g + cell - a.W) != kNone) ok &= uf_unite<kDev>(g, cell, cell - a.W, cells);
    if (x < a.W - 1 && (right || top) && lab_load<kDev>(g + cell - a.W + 1) != kNone)
      ok &= uf_unite<kDev>(g, cell, cell - a.W + 1, cells);
  }
  if (!ok) atomicOr(err, 1);
}

// --------------------------------------------------------------------------------- flatten
__global__ void __launch_bounds__(kBlock) cluster_flatten_kernel(int* __restrict__ cnt, int* __restrict__ lab,
                                                                 ClusterArgs a, int* __restrict__ err) {
  constexpr int kDev = __HIP_MEMORY_SCOPE_AGENT;
  const int cells = a.W * a.H;
  const int cell = blockIdx.x * kBlock + threadIdx.x;
  if (cell >= cells) return;
  int* g = lab + (long)blockIdx.y * cells;
  int* c = cnt + (long)blockIdx.y * cells;
  if (lab_load<kDev>(g + cell) == kNone) return;
  const int r = uf_find<kDev>(g, cell, cells);
  if (r < 0) { atomicOr(err, 1); return; }
  if (r == cell) return;
  // a shorter path to the same root: other lanes' finds may read either value
  __hip_atomic_store(g + cell, r, __ATOMIC_RELAXED, kDev);
  atomicAdd(c + r, c[cell]);  // only roots are added to, only other cells are read
}

// ------------------------------------------------------------------------------------ rank
__device__ __forceinline__ bool kept_root(const int* g, const int* c, int cell, int cells, const ClusterArgs& a) {
  if (cell >= cells || g[cell] != cell) return false;
  const int size = c[cell];
  return size >= a.min_pts && size <= a.max_pts;
}

// blocks: int32[B][nblk + 1], nblk = ceil(W * H / 256): per block its kept roots.
__global__ void __launch_bounds__(kBlock) cluster_rank_count_kernel(const int* __restrict__ cnt,
                                                                    const int* __restrict__ lab, ClusterArgs a,
                                                                    int* __restrict__ blocks) {
  __shared__ int w_cnt[kWaves];
  const int cells = a.W * a.H;
  const long plane = (long)blockIdx.y * cells;
  const bool kept = kept_root(lab + plane, cnt + plane, blockIdx.x * kBlock + threadIdx.x, cells, a);
  const unsigned long long m = __ballot(kept);
  if ((threadIdx.x & 63) == 0) w_cnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
    for (int w = 0; w < kWaves; ++w) n += w_cnt[w];
    blocks[(long)blockIdx.y * (gridDim.x + 1) + blockIdx.x] = n;
  }
}

// One workgroup per cloud: the block counts become exclusive prefixes in place; the total is `found`.
__global__ void __launch_bounds__(kBlock) cluster_rank_scan_kernel(int nblk, int* __restrict__ blocks,
                                                                   int* __restrict__ found) {
  __shared__ int sum[kBlock];
  const int b = blockIdx.x, t = threadIdx.x;
  int* mine = blocks + (long)b * (nblk + 1);
  const int chunk = (nblk + kBlock - 1) / kBlock;
  const int lo = min(t * chunk, nblk), hi = min(lo + chunk, nblk);
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
  if (t == kBlock - 1) {
    mine[nblk] = sum[t];
    found[b] = sum[t];
  }
}

__global__ void __launch_bounds__(kBlock) cluster_rank_assign_kernel(int* __restrict__ cnt,
                                                                     const int* __restrict__ lab, ClusterArgs a,
                                                                     const int* __restrict__ blocks,
                                                                     Row* __restrict__ table) {
  __shared__ int w_cnt[kWaves];
  const int cells = a.W * a.H;
  const long plane = (long)blockIdx.y * cells;
  const int cell = blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const bool kept = kept_root(lab + plane, cnt + plane, cell, cells, a);
  const unsigned long long m = __ballot(kept);
  if (lane == 0) w_cnt[wid] = __popcll(m);
  __syncthreads();
  if (cell >= cells || lab[plane + cell] != cell) return;  // not a root: its cnt is not read again
  int k = -1;
  if (kept) {
    k = blocks[(long)blockIdx.y * (gridDim.x + 1) + blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wid; ++w) k += w_cnt[w];
    if (k < a.max_k) table[(long)blockIdx.y * a.max_k + k].root = cell;
  }
  cnt[plane + cell] = k;
}

// ----------------------------------------------------------------------------------- stats
__device__ __forceinline__ void row_add(Row* r, int n, int x0, int x1, int y0, int y1, int z0, int z1, int sx,
                                        int sy, int sz) {
  atomicAdd(&r->n, n);
  atomicMin(&r->min_x, x0); atomicMax(&r->max_x, x1);
  atomicMin(&r->min_y, y0); atomicMax(&r->max_y, y1);
  atomicMin(&r->min_z, z0); atomicMax(&r->max_z, z1);
  atomicAdd((unsigned long long*)&r->sum_x, (unsigned long long)(long long)sx);
  atomicAdd((unsigned long long*)&r->sum_y, (unsigned long long)(long long)sy);
  atomicAdd((unsigned long long*)&r->sum_z, (unsigned long long)(long long)sz);
}

template <bool kAggregate>
__global__ void __launch_bounds__(kBlock) cluster_stats_kernel(
    const uint8_t* __restrict__ data, long data_bytes, const long* __restrict__ frame_off,
    const int* __restrict__ frame_n, ClusterArgs a, const int* __restrict__ cnt, const int* __restrict__ lab,
    const int* __restrict__ pcell, int* __restrict__ label, Row* __restrict__ table) {
  const int b = blockIdx.y;
  const int n_pts = cloud_points(frame_n, b, a);
  if ((long)blockIdx.x * kBlock >= n_pts) return;  // the whole workgroup
  const long foff = frame_off[b];
  const int path = cloud_frame_path(a.fast, foff);
  const long plane = (long)b * a.W * a.H;
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  float x = 0.f, y = 0.f, z = 0.f;
  int k = -1;
  if (load_point(data, data_bytes, foff, i, n_pts, a, path, &x, &y, &z)) {
    const long rec = (foff + i * a.step) / a.step;
    const int cell = pcell[rec];
    if (cell >= 0 && cell < a.W * a.H) {
      const int r = lab[plane + cell];
      if (r != kNone) k = cnt[plane + r];
      if (k >= a.max_k) k = -1;
    }
    label[rec] = k;
  }
  // a point with a cell is valid: |v| <= 512, the products are exact and below 2^19 + 1 in magnitude
  const int xi = k >= 0 ? (int)rintf(x * 1024.f) : 0, yi = k >= 0 ? (int)rintf(y * 1024.f) : 0,
            zi = k >= 0 ? (int)rintf(z * 1024.f) : 0;
  Row* rows = table + (long)b * a.max_k;
  if (!kAggregate) {
    if (k >= 0) row_add(rows + k, 1, xi, xi, yi, yi, zi, zi, xi, yi, zi);
    return;
  }
  if (__ballot(k >= 0) == 0ull) return;  // (the whole wave)
  const Run r = wave_run(k);
  int x0 = xi, x1 = xi, y0 = yi, y1 = yi, z0 = zi, z1 = zi, sx = xi, sy = yi, sz = zi;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {  // lane p of a run ends with the reduction of [p, len)
    const int tx0 = __shfl_down(x0, o, 64), tx1 = __shfl_down(x1, o, 64), ty0 = __shfl_down(y0, o, 64),
              ty1 = __shfl_down(y1, o, 64), tz0 = __shfl_down(z0, o, 64), tz1 = __shfl_down(z1, o, 64),
              tsx = __shfl_down(sx, o, 64), tsy = __shfl_down(sy, o, 64), tsz = __shfl_down(sz, o, 64);
    if (k >= 0 && r.pos + o < r.len) {
      x0 = min(x0, tx0); x1 = max(x1, tx1);
      y0 = min(y0, ty0); y1 = max(y1, ty1);
      z0 = min(z0, tz0); z1 = max(z1, tz1);
      sx += tsx; sy += tsy; sz += tsz;
    }
  }
  if (r.head) row_add(rows + k, r.len, x0, x1, y0, y1, z0, z1, sx, sy, sz);
}

}  // namespace

// data: device bytes, data_bytes of them (no record outside is read); frame_off long[B] (bytes): device; frame_n:
// device int32, cloud b's point count at frame_n[b * n_stride] (n_stride 1: a staged frame_n; 2: K30's counts, with
// data K30's output slab); max_n: the largest count the host knows (sizes the grids; the kernels clamp to it); offsets
// of x, y, z in a record of FLOAT32 fields.  x_min, y_min, cell, z_min, z_max: the float32 values of ops/cluster.py;
// W x H cells.  aggregate: 1, a wave's runs of equal k are reduced before the table's atomics; 0, one set per point.
// Workspace: cnt and lab int32[B * H * W], pcell int32[data_bytes / point_step + 1], blocks
// int32[B][ceil(W * H / 256) + 1].  Outputs: label int32[data_bytes / point_step + 1] (the record at byte `at` of data
// has index at / point_step), table B * max_clusters rows of 64 bytes, found int32[B] (uncapped), err int32[1] (not 0:
// a union-find loop hit its bound; the outputs are not to be used).
TCA_API int tca_cluster(const void* data, long data_bytes, const long* frame_off, const int* frame_n, int n_stride,
                        int batch, int max_n, int point_step, int off_x, int off_y, int off_z, float x_min,
                        float y_min, float cell, int W, int H, float z_min, float z_max, int min_cell_points,
                        int min_points, int max_points, int max_clusters, int aggregate, void* cnt, void* lab,
                        void* pcell, void* blocks, void* label, void* table, void* found, void* err,
                        hipStream_t stream) {
  if (batch < 1 || batch > kMaxFrames || max_n < 0 || point_step <= 0 || data_bytes < 0 ||
      data_bytes >= 0x80000000L || (n_stride != 1 && n_stride != 2) || (aggregate != 0 && aggregate != 1))
    return (int)hipErrorInvalidValue;
  if (W < 1 || W > kMaxSide || H < 1 || H > kMaxSide || (long)W * H > kMaxCells ||
      (long)batch * W * H > kMaxPlane || max_clusters < 1 || max_clusters > kMaxClusters)
    return (int)hipErrorInvalidValue;
  if (!std::isfinite(cell) || !(cell > 0.f) || !std::isfinite(x_min) || !std::isfinite(y_min) ||
      !std::isfinite(z_min) || !std::isfinite(z_max) || !(z_min <= z_max))
    return (int)hipErrorInvalidValue;
  if (min_cell_points < 1 || min_points < 1 || max_points < min_points) return (int)hipErrorInvalidValue;
  if (frame_off == nullptr || frame_n == nullptr || cnt == nullptr || lab == nullptr || pcell == nullptr ||
      blocks == nullptr || label == nullptr || table == nullptr || found == nullptr || err == nullptr ||
      (max_n > 0 && data == nullptr))
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)cnt & 3) != 0 || ((uintptr_t)lab & 3) != 0 || ((uintptr_t)pcell & 3) != 0 ||
      ((uintptr_t)blocks & 3) != 0 || ((uintptr_t)label & 3) != 0 || ((uintptr_t)table & 7) != 0 ||
      ((uintptr_t)found & 3) != 0 || ((uintptr_t)err & 3) != 0 || ((uintptr_t)frame_off & 7) != 0 ||
      ((uintptr_t)frame_n & 3) != 0)
    return (int)hipErrorInvalidValue;
  ClusterArgs a;
  a.step = point_step;
  a.off[0] = off_x; a.off[1] = off_y; a.off[2] = off_z; a.off[3] = -1;
  a.fast = cloud_fast_path(data, point_step, a.off, true);
  if (a.fast < 0) return (int)hipErrorInvalidValue;
  a.W = W; a.H = H; a.max_n = max_n; a.n_stride = n_stride;
  a.x0 = x_min; a.y0 = y_min; a.c32 = cell; a.z0 = z_min; a.z1 = z_max;
  a.min_cell = min_cell_points; a.min_pts = min_points; a.max_pts = max_points; a.max_k = max_clusters;

  const uint8_t* in = (const uint8_t*)data;
  const int cells = W * H, plane = batch * cells, rows = batch * max_clusters;  // <= 2^24, <= 2^18
  const int nblk = (cells + kBlock - 1) / kBlock;
  const int n_reset = std::max(plane, rows);
  cluster_reset_kernel<<<(unsigned)((n_reset + kBlock - 1) / kBlock), kBlock, 0, stream>>>(
      (int*)cnt, (int*)lab, plane, (Row*)table, rows, (int*)found, batch, (int*)err);
  if (max_n > 0) {
    if (int e = (int)hipGetLastError()) return e;
    const dim3 pgrid((max_n + kBlock - 1) / kBlock, batch), cgrid(nblk, batch);
    const dim3 tgrid(((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile), batch);
    cluster_count_kernel<<<pgrid, kBlock, 0, stream>>>(in, data_bytes, frame_off, frame_n, a, (int*)cnt,
                                                       (int*)pcell);
    if (int e = (int)hipGetLastError()) return e;
    cluster_tiles_kernel<<<tgrid, kBlock, 0, stream>>>((const int*)cnt, (int*)lab, a, (int*)err);
    if (int e = (int)hipGetLastError()) return e;
    cluster_merge_kernel<<<cgrid, kBlock, 0, stream>>>((int*)lab, a, (int*)err);
    if (int e = (int)hipGetLastError()) return e;
    cluster_flatten_kernel<<<cgrid, kBlock, 0, stream>>>((int*)cnt, (int*)lab, a, (int*)err);
    if (int e = (int)hipGetLastError()) return e;
    cluster_rank_count_kernel<<<cgrid, kBlock, 0, stream>>>((const int*)cnt, (const int*)lab, a, (int*)blocks);
    if (int e = (int)hipGetLastError()) return e;
    cluster_rank_scan_kernel<<<batch, kBlock, 0, stream>>>(nblk, (int*)blocks, (int*)found);
    if (int e = (int)hipGetLastError()) return e;
    cluster_rank_assign_kernel<<<cgrid, kBlock, 0, stream>>>((int*)cnt, (const int*)lab, a, (const int*)blocks,
                                                             (Row*)table);
    if (int e = (int)hipGetLastError()) return e;
    if (aggregate)
      cluster_stats_kernel<true><<<pgrid, kBlock, 0, stream>>>(in, data_bytes, frame_off, frame_n, a,
                                                               (const int*)cnt, (const int*)lab, (const int*)pcell,
                                                               (int*)label, (Row*)table);
    else
      cluster_stats_kernel<false><<<pgrid, kBlock, 0, stream>>>(in, data_bytes, frame_off, frame_n, a,
                                                                (const int*)cnt, (const int*)lab,
                                                                (const int*)pcell, (int*)label, (Row*)table);
  }
  TCA_LAUNCH_CHECK();
}
