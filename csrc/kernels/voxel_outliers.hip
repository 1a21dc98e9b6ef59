// K36 — outlier removal on the thinned cloud: pcl_ros's RadiusOutlierRemoval and StatisticalOutlierRemoval between
// tca_voxel_downsample and tca_voxel_normals.  ops/voxel_downsample.py (outliers_numpy) has the definition; these
// kernels give its bytes.  They run on the stream behind tca_voxel_downsample, read its records and counts[b] from the
// device and leave the kept records, in their order, and the new counts[b] where tca_voxel_normals and the fetch read
// them: no host round trip lies between the three.
//
// Per voxel a: q = rint(c * 65536) of its published float32 centroid; its neighbours are the voxels b != a of the same
// cloud with sum (q_b - q_a)^2 <= R^2 in int64 (a closed ball, itself excluded), `found` of them.  found = 0: gone.
// Radius test: found >= N.  Statistical test: the f = min(k, found) smallest D^2, e_j = rint(sqrt(f64(D^2_j))),
// mean = rint(f64(sum e_j) / f64(f)); over the n voxels with a neighbour S1 = sum mean, S2 = sum mean^2 (int64), and
// thr = S1 / n + stddev * sqrt(max((S2 - S1 S1 / n) / (n - 1), 0)) in float64; kept iff f64(mean) <= thr (n < 2: kept).
// Only the values of the k smallest D^2 are used, so neither the order of the cells nor ties reach an output byte.
//
// Workspace.  The leaf table of tca_voxel_downsample, dead after its scatter, holds the cell lists of side R
// (tca_cell_lists.h) and behind them three int64 per cloud (S1, S2, n), the clouds' cursors and the keys pass's
// (slot, rank) per row.  memo (int32 per staged point, dead too) takes the score of a row: -1 for no neighbour, else
// mean | min(found, 1023) << 20 (mean <= R <= 2^18, N <= 1000), and after the mark pass the row's rank among its
// block's survivors (-1: gone).  blocks int32[B][nblk + 1] takes the per-block survivor counts, then their exclusive
// prefixes, and in its spare last entry the cloud's records before the filter, which the scatter needs after counts[b]
// holds the survivors.
//
//   lists    reset, keys, starts, sort: tca_cell_lists.h.
//   score    one lane per record in cell order.  The lane probes the 27 cells around its own and streams their quads
//            from global memory (the walk the normals measured faster than staging through LDS); the kCap smallest D^2
//            stay in registers, sorted, and a candidate is inserted with kCap unrolled min / max pairs — no dynamic
//            index, no scratch.  kCap is k rounded up to 4, 8 or 16 (0: the radius test alone); unused entries are
//            +inf and never read.  The score goes to the record's ROW, so the later passes run in row order.  With
//            k > 0 the wave adds mean, mean^2 and 1 over its lanes with shuffles: one 64-bit atomic add per wave and sum.
//   mark     256 rows a workgroup in row order.  Every lane derives thr itself from S1, S2, n — a handful of float64
//            operations, the same for all — takes the keep decision, a ballot rank inside its wave and the workgroup
//            adds its four waves' counts.
//   scan     one workgroup per cloud: exclusive prefix over the block counts in place, the total into counts[b].
//   scatter  a kept row copies its record to the cloud's slot in `kept` at prefix + rank.
//
// No workgroup waits on another, only integer atomics are used, the resets belong to the launch (a relaunch or a graph
// replay gives the same bytes), nothing is allocated and no hipMemset is used.  Contraction to FMA is switched off for
// this file; division and square root are IEEE.
#include "tca_cell_lists.h"

#include <cmath>

#pragma clang fp contract(off)

using namespace tca;

namespace {

constexpr int kBlock = kCellBlock;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxNeighbors = 1000;  // ops/voxel_downsample.py OUTLIER_NEIGHBORS
constexpr int kMaxK = 16;            // OUTLIER_K
constexpr int kFoundShift = 20, kFoundMax = 1023, kMeanMask = (1 << kFoundShift) - 1;
constexpr long long kFar = 0x7FFFFFFFFFFFFFFFll;

__device__ __forceinline__ long long wave_sum64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int kCap>
__global__ void __launch_bounds__(kBlock) outliers_score_kernel(const int* __restrict__ counts, CellArgs a, int k,
                                                                const Cell* __restrict__ cells,
                                                                const int4* __restrict__ sorted, int* __restrict__ memo,
                                                                unsigned long long* __restrict__ stats) {
  const int b = blockIdx.y;
  const int K = records_of(counts, a, b);
  const long first = (long)blockIdx.x * kBlock;
  if (first >= K) return;  // the whole workgroup
  const Cell* tab = cells + a.slot_off[b];
  const int4* srt = sorted + a.pt_off[b];
  const int mask = a.mask[b], R = a.radius;
  const long long r2 = (long long)R * R;

  bool active = first + threadIdx.x < K;
  const int4 me = active ? srt[first + threadIdx.x] : make_int4(0, 0, 0, -1);
  active = active && me.w >= 0 && me.w < K;
  int found = 0;
  long long top[kCap > 0 ? kCap : 1];  // ascending
#pragma unroll
  for (int j = 0; j < kCap; ++j) top[j] = kFar;

  if (active) {
    const int cx = floor_div(me.x, R), cy = floor_div(me.y, R), cz = floor_div(me.z, R);
    for (int c = 0; c < 27; ++c) {
      int start = 0;
      const int count = find_cell(tab, mask, cell_key(cx + c % 3 - 1, cy + c / 3 % 3 - 1, cz + c / 9 - 1), K, &start);
      for (int e = 0; e < count; ++e) {
        const int4 it = srt[start + e];
        const int dx = it.x - me.x, dy = it.y - me.y, dz = it.z - me.z;  // |q| <= 2^25: no overflow
        long long d2 = (long long)dx * dx + (long long)dy * dy + (long long)dz * dz;
        if (d2 > r2 || it.w == me.w) continue;
        found += 1;
        if (kCap > 0 && d2 < top[kCap > 0 ? kCap - 1 : 0]) {
#pragma unroll
          for (int j = 0; j < kCap; ++j) {  // the candidate sinks to its place, the largest falls off the end
            const long long lo = d2 < top[j] ? d2 : top[j];
            d2 = d2 < top[j] ? top[j] : d2;
            top[j] = lo;
          }
        }
      }
    }
  }

  long long mean = 0;
  if (kCap > 0 && found > 0) {
    const int f = min(k, found);
    long long sum = 0;
#pragma unroll
    for (int j = 0; j < kCap; ++j)
      if (j < f) sum += (long long)rint(sqrt((double)top[j]));  // D^2 < 2^37: exact in float64
    mean = (long long)rint((double)sum / (double)f);
  }
  if (active) memo[a.pt_off[b] + me.w] = found > 0 ? ((int)mean | (min(found, kFoundMax) << kFoundShift)) : -1;
  if (kCap > 0) {  // (every lane of the wave is here: no early return above)
    const long long has = found > 0 ? 1 : 0;
    const long long s1 = wave_sum64(mean), s2 = wave_sum64(mean * mean), n = wave_sum64(has);
    if ((threadIdx.x & 63) == 0 && n > 0) {
      atomicAdd(&stats[3 * b + 0], (unsigned long long)s1);
      atomicAdd(&stats[3 * b + 1], (unsigned long long)s2);
      atomicAdd(&stats[3 * b + 2], (unsigned long long)n);
    }
  }
}

__global__ void __launch_bounds__(kBlock) outliers_mark_kernel(const int* __restrict__ counts, CellArgs a, int min_nb,
                                                               int k, double stddev,
                                                               const unsigned long long* __restrict__ stats,
                                                               int* __restrict__ memo, int* __restrict__ blocks) {
  __shared__ int w_cnt[kWaves];
  const int b = blockIdx.y;
  const int K = records_of(counts, a, b);
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if ((long)blockIdx.x * kBlock >= K) return;
  const int nblk = (a.max_n + kBlock - 1) / kBlock;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;

  const int score = i < K ? memo[a.pt_off[b] + i] : -1;
  const int found = score < 0 ? 0 : score >> kFoundShift;
  bool keep = found >= 1 && found >= min_nb;
  if (k > 0) {
    const long long n = (long long)stats[3 * b + 2];
    if (n >= 2) {
      const double s1 = (double)(long long)stats[3 * b + 0], s2 = (double)(long long)stats[3 * b + 1], fn = (double)n;
      const double mu = s1 / fn;
      const double var = (s2 - (s1 * s1) / fn) / (fn - 1.0);
      const double thr = mu + stddev * sqrt(var > 0.0 ? var : 0.0);
      keep = keep && (double)(score & kMeanMask) <= thr;
    }
  }
  const unsigned long long w = __ballot(keep);
  if (lane == 0) w_cnt[wid] = __popcll(w);
  __syncthreads();
  int rank = __popcll(w & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
  for (int j = 0; j < kWaves; ++j) {
    if (j < wid) rank += w_cnt[j];
    total += w_cnt[j];
  }
  if (i < K) memo[a.pt_off[b] + i] = keep ? rank : -1;
  if (threadIdx.x == 0) blocks[(long)b * (nblk + 1) + blockIdx.x] = total;
}

// One workgroup per cloud: the block counts become exclusive prefixes in place, the total goes into counts[b] and the
// records the cloud had before into the spare entry behind its blocks.
__global__ void __launch_bounds__(kBlock) outliers_scan_kernel(CellArgs a, int* __restrict__ blocks,
                                                               int* __restrict__ counts) {
  __shared__ int sum[kBlock];
  const int b = blockIdx.x, t = threadIdx.x;
  const int nblk = (a.max_n + kBlock - 1) / kBlock;
  const int K = records_of(counts, a, b);
  const int n_blocks = (K + kBlock - 1) / kBlock;
  int* mine = blocks + (long)b * (nblk + 1);
  const int chunk = (n_blocks + kBlock - 1) / kBlock;
  const int lo = min(t * chunk, n_blocks), hi = min(lo + chunk, n_blocks);
  int own = 0;
  for (int j = lo; j < hi; ++j) own += mine[j];
  sum[t] = own;
  __syncthreads();  // (every thread has read counts[b] by now)
  for (int o = 1; o < kBlock; o <<= 1) {  // inclusive, over the threads' chunks
    const int v = t >= o ? sum[t - o] : 0;
    __syncthreads();
    sum[t] += v;
    __syncthreads();
  }
  int run = sum[t] - own;
  for (int j = lo; j < hi; ++j) {
    const int c = mine[j];
    mine[j] = run;
    run += c;
  }
  if (t == kBlock - 1) {
    counts[b] = sum[t];
    mine[nblk] = K;
  }
}

__global__ void __launch_bounds__(kBlock) outliers_scatter_kernel(const uint4* __restrict__ rows, CellArgs a,
                                                                  const int* __restrict__ blocks,
                                                                  const int* __restrict__ memo, uint4* __restrict__ kept,
                                                                  long n_records) {
  const int b = blockIdx.y;
  const int nblk = (a.max_n + kBlock - 1) / kBlock;
  const int* mine = blocks + (long)b * (nblk + 1);
  const int K = min(max(mine[nblk], 0), a.n[b]);
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= K) return;
  const int rank = memo[a.pt_off[b] + i];
  if (rank < 0 || rank >= kBlock) return;
  const long at = (long)mine[blockIdx.x] + rank;  // a survivor never moves up: at <= i
  const long to = (long)a.pt_off[b] + at;
  if (at >= 0 && at <= i && to < n_records) kept[to] = rows[a.pt_off[b] + i];
}

}  // namespace

// rows: the 16-byte records tca_voxel_downsample wrote (device, 16-byte aligned, rows_bytes >= 16 * sum(ns)), cloud
// b's from record sum(ns[:b]); counts int[B] (device): the records of every cloud, clamped to ns[b]; on return of the
// work the survivors of every cloud.  ns, slots: HOST int[B], what tca_voxel_downsample took.  radius_q: the ball's
// radius in units of 2^-16 m, 1..4 * 65536.  min_neighbors: 0 (off) or 1..1000; mean_k: 0 (off) or 1..16, one of the
// two on; stddev: 0..10.  table: the leaf table's bytes (48 * sum(slots), 16-byte aligned), memo int32[sum(ns)], blocks
// int32[B][ceil(max(ns) / 256) + 1]: tca_voxel_downsample's, dead after it, reset here on the stream where they must
// be.  kept: 16-byte records like rows (another buffer), kept_bytes >= 16 * sum(ns), 16-byte aligned; only the first
// counts[b] of a cloud are written.  A buffer shorter than that, or misaligned, is refused, and nothing is launched.
TCA_API int tca_voxel_outliers(const void* rows, long rows_bytes, int* counts, const int* ns, const int* slots,
                               int batch, int radius_q, int min_neighbors, int mean_k, double stddev, void* table,
                               long table_bytes, void* memo, long memo_bytes, void* blocks, long blocks_bytes,
                               void* kept, long kept_bytes, hipStream_t stream) {
  if (min_neighbors < 0 || min_neighbors > kMaxNeighbors || mean_k < 0 || mean_k > kMaxK ||
      (min_neighbors == 0 && mean_k == 0) || !(stddev >= 0.0 && stddev <= 10.0))  // (a NaN compares false)
    return (int)hipErrorInvalidValue;
  if (batch < 1 || batch > kCellFrames) return (int)hipErrorInvalidValue;
  const int front = 6 * batch;  // S1, S2, n: three int64 per cloud, zeroed with the cursors
  CellPlan p;
  if (!cell_plan(ns, slots, batch, radius_q, front, table, table_bytes, p)) return (int)hipErrorInvalidValue;
  const int nblk = (p.a.max_n + kBlock - 1) / kBlock;
  // the keys pass's (slot, rank) behind the zeroed ints: 16 (slots + 2 n) + 32 B <= 48 slots, as slots >= max(n, 2)
  const long scratch_at = 16 * (p.slot_sum + p.n_sum) + 16 * ((4L * (front + batch) + 15) / 16);
  if (scratch_at + 16 * p.n_sum > table_bytes || rows_bytes < 16 * p.n_sum || kept_bytes < 16 * p.n_sum ||
      memo_bytes < 4 * p.n_sum || blocks_bytes < 4L * batch * (nblk + 1))
    return (int)hipErrorInvalidValue;
  if (rows == nullptr || counts == nullptr || memo == nullptr || blocks == nullptr || kept == nullptr || rows == kept)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)rows & 15) != 0 || ((uintptr_t)kept & 15) != 0 || ((uintptr_t)counts & 3) != 0 ||
      ((uintptr_t)memo & 3) != 0 || ((uintptr_t)blocks & 3) != 0)
    return (int)hipErrorInvalidValue;
  if (p.a.max_n == 0) return (int)hipSuccess;

  const uint4* in = (const uint4*)rows;
  unsigned long long* stats = (unsigned long long*)p.zeroed;
  uint4* scratch = (uint4*)((uint8_t*)table + scratch_at);
  if (int e = cell_lists_build(p, in, counts, batch, front, scratch, stream)) return e;
  const dim3 grid(nblk, batch);
  if (mean_k == 0)
    outliers_score_kernel<0><<<grid, kBlock, 0, stream>>>(counts, p.a, mean_k, p.cells, p.sorted, (int*)memo, stats);
  else if (mean_k <= 4)
    outliers_score_kernel<4><<<grid, kBlock, 0, stream>>>(counts, p.a, mean_k, p.cells, p.sorted, (int*)memo, stats);
  else if (mean_k <= 8)
    outliers_score_kernel<8><<<grid, kBlock, 0, stream>>>(counts, p.a, mean_k, p.cells, p.sorted, (int*)memo, stats);
  else
    outliers_score_kernel<16><<<grid, kBlock, 0, stream>>>(counts, p.a, mean_k, p.cells, p.sorted, (int*)memo, stats);
  if (int e = (int)hipGetLastError()) return e;
  outliers_mark_kernel<<<grid, kBlock, 0, stream>>>(counts, p.a, min_neighbors, mean_k, stddev, stats, (int*)memo,
                                                    (int*)blocks);
  if (int e = (int)hipGetLastError()) return e;
  outliers_scan_kernel<<<batch, kBlock, 0, stream>>>(p.a, (int*)blocks, counts);
  if (int e = (int)hipGetLastError()) return e;
  outliers_scatter_kernel<<<grid, kBlock, 0, stream>>>(in, p.a, (const int*)blocks, (const int*)memo, (uint4*)kept,
                                                       p.n_sum);
  TCA_LAUNCH_CHECK();
}
