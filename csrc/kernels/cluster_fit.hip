// K32 — an oriented box per obstacle cluster: the search-based L-shape fit with the closeness criterion, in
// integers (ops/cluster_fit.py has the definition).  It runs on the stream behind K31 (cluster.hip) and reads what
// K31 read and wrote where it lies: the records, the per-record label, the table and found.
//
// Per cluster, every point is projected onto `angles` <= 128 candidate directions twice: once for the four bounds of
// each direction, once for the closeness sum that needs those bounds.  Clusters run from a handful of points to tens
// of thousands in one cloud, so the work is first grouped by cluster and then split by size:
//
//   plan     one workgroup per cloud scans the table's n over min(found, max_clusters) rows into offsets into the
//            grouped point buffer (an oversize cluster: length 0 and its flag row), and in the same pass numbers the
//            clusters of more than CHUNK points (their slots), lists their chunks and resets the slots' rows.  Rows
//            from min(found, max_clusters) on are zeroed.
//   group    one lane per record: k = label[rec], xi, yi as K31's stats kernel makes them, minus the cluster's
//            centre, stored at the cluster's offset plus a cursor; a wave's run of equal k takes one cursor atomic.
//            The order inside a cluster is whatever the atomics give; no output depends on it.
//   fit      one workgroup per cluster of at most CHUNK points.  Its (dx, dy) are loaded into LDS once (32 KiB).
//            Threads own directions, not points: thread t has direction t & 127 and takes the points of parity
//            t >> 7, so every lane of a wave reads the same LDS address per step (a broadcast, no bank conflict) and
//            keeps its direction's four bounds in registers.  The two halves are combined through LDS, a second
//            sweep over the same LDS points sums the closeness weights (a chunk's sum fits 32 bits: 4096 * 65536),
//            and wave 0 reduces over the directions for the winner and writes the row.  Nothing goes through global
//            memory in between.
//   bounds,  the clusters of more than CHUNK points (a wall, a hedge), one workgroup per chunk of CHUNK points so
//   score,   that no cloud waits for one long workgroup: the bounds go by atomicMin / atomicMax into the slot's row
//   select   of the direction, in a second launch the closeness sums by 64-bit atomicAdd, and a third selects each
//            slot's winner.  A cloud of max_n points has at most max_n / CHUNK such clusters.
//
// split = 0 gives every cluster to `fit`, which then walks the chunks itself (measurements).  Both give the same
// bytes: every reduction is an integer minimum, maximum or sum.
//
// Nothing is allocated, no hipMemset is used, only integer atomics; everything a launch reads it has written
// itself or K31 has; no workgroup waits on another.  Every index into the grouped buffer is bounded by what the
// plan derived from the buffer's size, whatever the table holds.
#include "tca_cloud_load.h"
#include "tca_cluster.h"
#include "tca_common.h"

#pragma clang fp contract(off)

using namespace tca;

namespace {

constexpr int kBlock = 256;
constexpr int kChunk = 4096;
constexpr int kMaxAngles = 128;
constexpr int kMaxFrames = 64;
constexpr int kMaxClusters = 4096;
constexpr int kMaxSide = 65536;  // units of 1/1024 m
constexpr int kNone = 0x7FFFFFFF;
constexpr int kIntMin = -0x7FFFFFFF - 1;

struct FitArgs {
  int step;
  int off[4];  // x, y, z, -1
  int fast;    // tca_cloud_load.h
  int max_n, n_stride, max_k, angles, d0q, split;
  int cap;      // slots per cloud: max_n / CHUNK + 1
  int records;  // of the grouped buffer and of label
  int cs[2 * kMaxAngles];  // c_j at j, s_j at 128 + j
};

struct Plan {  // 16 bytes per table row
  int off;     // of the cluster's first point in the grouped buffer
  int len;     // its points; 0: not fitted
  int slot;    // -1: at most CHUNK points
  int cursor;  // group: the points stored so far
};

struct FitRow {  // 32 bytes: ops/cluster_fit.py FIT_DTYPE
  int j, flags;
  int u_min, u_max, v_min, v_max;
  long long score;
};
static_assert(sizeof(FitRow) == 32, "a fit row is 32 bytes");

struct Slot {  // 32 bytes per cloud, slot and direction
  int u_min, u_max, v_min, v_max;
  long long score;
  long long pad;
};

struct Lds {
  int2 pts[kChunk];
  int bounds[2][kMaxAngles][4];
  long long score[2][kMaxAngles];
};

__device__ __forceinline__ int work_ints(const FitArgs& a) { return 2 + 5 * a.cap; }

// ------------------------------------------------------------------------------------ plan
// Exclusive prefix of `own` over the workgroup's threads; *total: the sum.  (Two barriers a step.)
template <typename T>
__device__ __forceinline__ T block_scan(T own, T* lds, T* total) {
  const int t = threadIdx.x;
  __syncthreads();  // lds may still be read from the scan before
  lds[t] = own;
  __syncthreads();
  for (int o = 1; o < kBlock; o <<= 1) {
    const T v = t >= o ? lds[t - o] : (T)0;
    __syncthreads();
    lds[t] += v;
    __syncthreads();
  }
  *total = lds[kBlock - 1];
  return lds[t] - own;
}

// The points of a row that is fitted, 0 for an oversize or empty one.
__device__ __forceinline__ int row_len(const Row& r, int n_cap) {
  if ((long)r.max_x - r.min_x > kMaxSide || (long)r.max_y - r.min_y > kMaxSide) return 0;
  return min(max(r.n, 0), n_cap);
}

__global__ void __launch_bounds__(kBlock) fit_plan_kernel(long data_bytes, const long* __restrict__ frame_off,
                                                          const int* __restrict__ frame_n,
                                                          const Row* __restrict__ table,
                                                          const int* __restrict__ found, FitArgs a,
                                                          Plan* __restrict__ plan, Slot* __restrict__ slots,
                                                          int* __restrict__ work, FitRow* __restrict__ fit) {
  __shared__ long long s_ll[kBlock];
  __shared__ int s_int[kBlock];
  const int b = blockIdx.x, t = threadIdx.x;
  const long foff = frame_off[b];
  const long rec0 = foff / a.step;
  int n_cap = 0;  // the cloud's records that lie inside the buffer
  if (foff >= 0 && foff <= data_bytes)
    n_cap = (int)max(min((long)min(max(frame_n[(long)b * a.n_stride], 0), a.max_n), (long)a.records - rec0), 0L);
  const int rows = min(max(found[b], 0), a.max_k);
  const Row* tab = table + (long)b * a.max_k;
  Plan* pl = plan + (long)b * a.max_k;
  FitRow* out = fit + (long)b * a.max_k;
  int* wk = work + (long)b * work_ints(a);
  const int per = (a.max_k + kBlock - 1) / kBlock;
  const int lo = min(t * per, rows), hi = min(lo + per, rows);

  long long own = 0;
  for (int k = lo; k < hi; ++k) own += row_len(tab[k], n_cap);
  long long all;
  const long long base = block_scan<long long>(own, s_ll, &all);

  // a row is fitted when its range lies inside the cloud's: such ranges are disjoint and sum to at most max_n,
  // so at most `cap` of them exceed CHUNK and they make at most 2 * cap chunks
  long long run = base;
  int n_slot = 0, n_chunk = 0;
  for (int k = lo; k < hi; ++k) {
    const int len = row_len(tab[k], n_cap);
    if (len > 0 && run + len <= n_cap && a.split && len > kChunk) {
      ++n_slot;
      n_chunk += (len + kChunk - 1) / kChunk;
    }
    run += len;
  }
  int slots_all, chunks_all;
  int sl = block_scan<int>(n_slot, s_int, &slots_all);
  int ch = block_scan<int>(n_chunk, s_int, &chunks_all);

  run = base;
  for (int k = lo; k < hi; ++k) {
    const int len = row_len(tab[k], n_cap);
    const bool ok = len > 0 && run + len <= n_cap;
    Plan p;
    p.off = (int)(rec0 + run);
    p.len = ok ? len : 0;
    p.slot = -1;
    p.cursor = 0;
    if (ok && a.split && len > kChunk) {
      p.slot = sl;
      wk[2 + sl] = k;
      const int m = (len + kChunk - 1) / kChunk;
      for (int c = 0; c < m; ++c) {
        wk[2 + a.cap + 2 * (ch + c)] = sl;
        wk[2 + a.cap + 2 * (ch + c) + 1] = c;
      }
      ++sl;
      ch += m;
    }
    pl[k] = p;
    if (!ok) {
      FitRow r;
      r.j = 0; r.flags = 1;
      r.u_min = r.u_max = r.v_min = r.v_max = 0;
      r.score = 0;
      out[k] = r;
    }
    run += len;
  }
  for (int k = rows + t; k < a.max_k; k += kBlock) {
    FitRow r;
    r.j = r.flags = r.u_min = r.u_max = r.v_min = r.v_max = 0;
    r.score = 0;
    out[k] = r;
  }
  if (t == 0) {
    wk[0] = slots_all;
    wk[1] = chunks_all;
  }
  Slot* mine = slots + (long)b * a.cap * a.angles;
  for (int i = t; i < slots_all * a.angles; i += kBlock) {
    Slot s;
    s.u_min = s.v_min = kNone;
    s.u_max = s.v_max = kIntMin;
    s.score = s.pad = 0;
    mine[i] = s;
  }
}

// ----------------------------------------------------------------------------------- group
__global__ void __launch_bounds__(kBlock) fit_group_kernel(
    const uint8_t* __restrict__ data, long data_bytes, const long* __restrict__ frame_off,
    const int* __restrict__ frame_n, const int* __restrict__ label, const Row* __restrict__ table,
    const int* __restrict__ found, FitArgs a, Plan* __restrict__ plan, int2* __restrict__ grouped) {
  const int b = blockIdx.y;
  const int n_pts = min(max(frame_n[(long)b * a.n_stride], 0), a.max_n);
  if ((long)blockIdx.x * kBlock >= n_pts) return;  // the whole workgroup
  const long foff = frame_off[b];
  const int path = cloud_frame_path(a.fast, foff);
  const int rows = min(max(found[b], 0), a.max_k);
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  const long at = foff + i * a.step;
  Plan* pl = plan + (long)b * a.max_k;
  int k = -1, dx = 0, dy = 0, off = 0, len = 0;
  if (i < n_pts && foff >= 0 && foff <= data_bytes && at + a.step <= data_bytes) {
    k = label[at / a.step];
    if (k >= rows) k = -1;
    if (k >= 0) {
      off = pl[k].off;
      len = pl[k].len;
      if (len == 0) k = -1;
    }
    if (k >= 0) {
      uint32_t raw[4] = {0u, 0u, 0u, 0u};
      cloud_load_fields(data + at, a.off, path, raw);
      const Row& r = table[(long)b * a.max_k + k];
      // a labelled point is valid: |v| <= 512, the products are exact
      dx = (int)rintf(__uint_as_float(raw[0]) * 1024.f) - ((r.min_x + r.max_x) >> 1);
      dy = (int)rintf(__uint_as_float(raw[1]) * 1024.f) - ((r.min_y + r.max_y) >> 1);
    }
  }
  if (__ballot(k >= 0) == 0ull) return;  // (the whole wave)
  const Run r = wave_run(k);
  int first = 0;
  if (r.head) first = atomicAdd(&pl[k].cursor, r.len);
  first = __shfl(first, (int)(threadIdx.x & 63) - r.pos, 64);  // the run's head
  if (k >= 0 && first >= 0 && first + r.pos < len) grouped[(long)off + first + r.pos] = make_int2(dx, dy);
}

// ------------------------------------------------------------------------------ the sweeps
__device__ __forceinline__ void load_chunk(Lds& s, const int2* __restrict__ src, int m) {
  for (int i = threadIdx.x; i < m; i += kBlock) s.pts[i] = src[i];
}

// Thread t: direction t & 127, the points of parity t >> 7.
__device__ __forceinline__ void sweep_bounds(const Lds& s, int m, int c, int sn, int (&bd)[4]) {
#pragma unroll 4
  for (int i = threadIdx.x >> 7; i < m; i += 2) {
    const int2 q = s.pts[i];
    const int u = q.x * c + q.y * sn, v = q.y * c - q.x * sn;
    bd[0] = min(bd[0], u); bd[1] = max(bd[1], u);
    bd[2] = min(bd[2], v); bd[3] = max(bd[3], v);
  }
}

// The closeness sum of the thread's points: at most 2048 * 65536.
__device__ __forceinline__ int sweep_score(const Lds& s, int m, int c, int sn, const int (&bd)[4], int d0q) {
  const unsigned num = (unsigned)d0q << 16;
  int sum = 0;
#pragma unroll 2
  for (int i = threadIdx.x >> 7; i < m; i += 2) {
    const int2 q = s.pts[i];
    const int u = q.x * c + q.y * sn, v = q.y * c - q.x * sn;
    const int d = min(min(u - bd[0], bd[1] - u), min(v - bd[2], bd[3] - v)) >> 10;
    sum += d <= d0q ? 65536 : (int)(num / (unsigned)d);
  }
  return sum;
}

// Both halves' bounds of every direction → the direction's bounds, in both.  (One barrier.)
__device__ __forceinline__ void combine_bounds(Lds& s, int (&bd)[4]) {
  const int j = threadIdx.x & 127, h = threadIdx.x >> 7;
#pragma unroll
  for (int e = 0; e < 4; ++e) s.bounds[h][j][e] = bd[e];
  __syncthreads();
  bd[0] = min(bd[0], s.bounds[h ^ 1][j][0]); bd[1] = max(bd[1], s.bounds[h ^ 1][j][1]);
  bd[2] = min(bd[2], s.bounds[h ^ 1][j][2]); bd[3] = max(bd[3], s.bounds[h ^ 1][j][3]);
}

// Is (score a, area a, ja) the better of two candidates: the larger score, then the smaller area, then the
// smaller direction.
__device__ __forceinline__ bool better(long long sa, long long aa, int ja, long long sb, long long ab, int jb) {
  return sa != sb ? sa > sb : aa != ab ? aa < ab : ja < jb;
}

// Wave 0: the winner of the directions whose bounds are in s.bounds[0] and whose score is s.score[0] + s.score[1];
// lane 0 writes the row.  (The caller has put a barrier behind those writes.)
__device__ __forceinline__ void select_write(const Lds& s, int angles, FitRow* __restrict__ out) {
  if (threadIdx.x >= 64) return;
  long long best_s = -1, best_a = 0;
  int best_j = kNone;
#pragma unroll
  for (int j = threadIdx.x; j < kMaxAngles; j += 64) {
    if (j >= angles) break;
    const long long sc = s.score[0][j] + s.score[1][j];
    const long long ar = ((long long)s.bounds[0][j][1] - s.bounds[0][j][0]) *
                         ((long long)s.bounds[0][j][3] - s.bounds[0][j][2]);
    if (better(sc, ar, j, best_s, best_a, best_j)) { best_s = sc; best_a = ar; best_j = j; }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const long long os = __shfl_down(best_s, o, 64), oa = __shfl_down(best_a, o, 64);
    const int oj = __shfl_down(best_j, o, 64);
    if (better(os, oa, oj, best_s, best_a, best_j)) { best_s = os; best_a = oa; best_j = oj; }
  }
  if (threadIdx.x == 0) {  // angles >= 2: lanes 0 and 1 had a direction
    FitRow r;
    r.j = best_j; r.flags = 0;
    r.u_min = s.bounds[0][best_j][0]; r.u_max = s.bounds[0][best_j][1];
    r.v_min = s.bounds[0][best_j][2]; r.v_max = s.bounds[0][best_j][3];
    r.score = best_s;
    *out = r;
  }
}

// ------------------------------------------------------------------------------------- fit
__global__ void __launch_bounds__(kBlock) fit_cluster_kernel(const int* __restrict__ found, FitArgs a,
                                                             const Plan* __restrict__ plan,
                                                             const int2* __restrict__ grouped,
                                                             FitRow* __restrict__ fit) {
  __shared__ Lds s;
  const int k = blockIdx.x, b = blockIdx.y;
  if (k >= min(max(found[b], 0), a.max_k)) return;
  const Plan p = plan[(long)b * a.max_k + k];
  if (p.len == 0 || p.slot >= 0) return;
  const int j = threadIdx.x & 127, h = threadIdx.x >> 7;
  const bool on = j < a.angles;
  const int c = on ? a.cs[j] : 0, sn = on ? a.cs[kMaxAngles + j] : 0;
  const int2* src = grouped + p.off;
  const int chunks = (p.len + kChunk - 1) / kChunk;  // 1 unless split = 0

  int bd[4] = {kNone, kIntMin, kNone, kIntMin};
  for (int ch = 0; ch < chunks; ++ch) {
    const int m = min(kChunk, p.len - ch * kChunk);
    if (ch > 0) __syncthreads();
    load_chunk(s, src + (long)ch * kChunk, m);
    __syncthreads();
    if (on) sweep_bounds(s, m, c, sn, bd);
  }
  combine_bounds(s, bd);
  long long sum = 0;
  for (int ch = 0; ch < chunks; ++ch) {
    const int m = min(kChunk, p.len - ch * kChunk);
    if (chunks > 1) {  // else the chunk is still there
      __syncthreads();
      load_chunk(s, src + (long)ch * kChunk, m);
      __syncthreads();
    }
    if (on) sum += sweep_score(s, m, c, sn, bd, a.d0q);
  }
  __syncthreads();  // every thread has read the other half's bounds
  s.score[h][j] = sum;
  if (h == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) s.bounds[0][j][e] = bd[e];
  }
  __syncthreads();
  select_write(s, a.angles, fit + (long)b * a.max_k + k);
}

// ------------------------------------------------------------------- clusters of many chunks
// The chunk of this workgroup: false past the cloud's list.
__device__ __forceinline__ bool chunk_of(const int* __restrict__ work, const FitArgs& a, const Plan* __restrict__ plan,
                                         int* slot, const int2** src, int* m, const int2* __restrict__ grouped) {
  const int b = blockIdx.y;
  const int* wk = work + (long)b * work_ints(a);
  if ((int)blockIdx.x >= wk[1]) return false;
  *slot = wk[2 + a.cap + 2 * blockIdx.x];
  const int ch = wk[2 + a.cap + 2 * blockIdx.x + 1];
  const Plan p = plan[(long)b * a.max_k + wk[2 + *slot]];
  *src = grouped + p.off + (long)ch * kChunk;
  *m = min(kChunk, p.len - ch * kChunk);
  return true;
}

__global__ void __launch_bounds__(kBlock) fit_chunk_bounds_kernel(FitArgs a, const Plan* __restrict__ plan,
                                                                  const int2* __restrict__ grouped,
                                                                  const int* __restrict__ work,
                                                                  Slot* __restrict__ slots) {
  __shared__ Lds s;
  int slot, m;
  const int2* src;
  if (!chunk_of(work, a, plan, &slot, &src, &m, grouped)) return;
  const int j = threadIdx.x & 127, h = threadIdx.x >> 7;
  const bool on = j < a.angles;
  const int c = on ? a.cs[j] : 0, sn = on ? a.cs[kMaxAngles + j] : 0;
  load_chunk(s, src, m);
  __syncthreads();
  int bd[4] = {kNone, kIntMin, kNone, kIntMin};
  if (on) sweep_bounds(s, m, c, sn, bd);
  combine_bounds(s, bd);
  if (on && h == 0) {
    Slot* row = slots + ((long)blockIdx.y * a.cap + slot) * a.angles + j;
    atomicMin(&row->u_min, bd[0]); atomicMax(&row->u_max, bd[1]);
    atomicMin(&row->v_min, bd[2]); atomicMax(&row->v_max, bd[3]);
  }
}

__global__ void __launch_bounds__(kBlock) fit_chunk_score_kernel(FitArgs a, const Plan* __restrict__ plan,
                                                                 const int2* __restrict__ grouped,
                                                                 const int* __restrict__ work,
                                                                 Slot* __restrict__ slots) {
  __shared__ Lds s;
  int slot, m;
  const int2* src;
  if (!chunk_of(work, a, plan, &slot, &src, &m, grouped)) return;
  const int j = threadIdx.x & 127, h = threadIdx.x >> 7;
  const bool on = j < a.angles;
  const int c = on ? a.cs[j] : 0, sn = on ? a.cs[kMaxAngles + j] : 0;
  Slot* row = slots + ((long)blockIdx.y * a.cap + slot) * a.angles + (on ? j : 0);
  const int bd[4] = {row->u_min, row->u_max, row->v_min, row->v_max};  // final since the launch before
  load_chunk(s, src, m);
  __syncthreads();
  const int sum = on ? sweep_score(s, m, c, sn, bd, a.d0q) : 0;
  s.score[h][j] = sum;
  __syncthreads();
  if (on && h == 0)
    atomicAdd((unsigned long long*)&row->score, (unsigned long long)(s.score[0][j] + s.score[1][j]));
}

__global__ void __launch_bounds__(kMaxAngles) fit_select_kernel(FitArgs a, const int* __restrict__ work,
                                                                const Slot* __restrict__ slots,
                                                                FitRow* __restrict__ fit) {
  __shared__ int s_bounds[kMaxAngles][4];
  __shared__ long long s_score[kMaxAngles];
  const int b = blockIdx.y, slot = blockIdx.x, j = threadIdx.x;
  const int* wk = work + (long)b * work_ints(a);
  if (slot >= wk[0]) return;
  if (j < a.angles) {
    const Slot r = slots[((long)b * a.cap + slot) * a.angles + j];
    s_bounds[j][0] = r.u_min; s_bounds[j][1] = r.u_max; s_bounds[j][2] = r.v_min; s_bounds[j][3] = r.v_max;
    s_score[j] = r.score;
  }
  __syncthreads();
  if (j >= 64) return;
  long long best_s = -1, best_a = 0;
  int best_j = kNone;
  for (int d = j; d < a.angles; d += 64) {
    const long long ar = ((long long)s_bounds[d][1] - s_bounds[d][0]) * ((long long)s_bounds[d][3] - s_bounds[d][2]);
    if (better(s_score[d], ar, d, best_s, best_a, best_j)) { best_s = s_score[d]; best_a = ar; best_j = d; }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const long long os = __shfl_down(best_s, o, 64), oa = __shfl_down(best_a, o, 64);
    const int oj = __shfl_down(best_j, o, 64);
    if (better(os, oa, oj, best_s, best_a, best_j)) { best_s = os; best_a = oa; best_j = oj; }
  }
  if (j == 0) {
    FitRow r;
    r.j = best_j; r.flags = 0;
    r.u_min = s_bounds[best_j][0]; r.u_max = s_bounds[best_j][1];
    r.v_min = s_bounds[best_j][2]; r.v_max = s_bounds[best_j][3];
    r.score = best_s;
    fit[(long)b * a.max_k + wk[2 + slot]] = r;
  }
}

}  // namespace

// data, data_bytes, frame_off, frame_n, n_stride, batch, max_n, point_step and the offsets: what tca_cluster took
// (off_z only classifies the layout).  label int32[data_bytes / point_step + 1], table batch * max_clusters rows of 64
// bytes and found int32[batch]: what it wrote.  angles in 2..128; d0q = rint(d0 * 2^14) in 164..16384; trig: HOST
// int32[2][angles], c_j then s_j, each within +-16384 (copied into the kernels' arguments here).  split: 1, clusters
// of more than 4096 points are fitted a chunk a workgroup; 0, one workgroup per cluster.  Workspace: plan 16 bytes per
// table row, grouped 8 bytes per record (data_bytes / point_step + 1), slots 32 bytes * batch * (max_n / 4096 + 1) *
// angles, work int32[batch][2 + 5 * (max_n / 4096 + 1)]; slots_bytes and work_bytes: what the two buffers hold, a
// shorter one is refused.  Output: fit, batch * max_clusters rows of 32 bytes; the
// rows from min(found, max_clusters) on are zero.
TCA_API int tca_cluster_fit(const void* data, long data_bytes, const long* frame_off, const int* frame_n, int n_stride,
                            int batch, int max_n, int point_step, int off_x, int off_y, int off_z, const void* label,
                            const void* table, const void* found, int max_clusters, int angles, int d0q,
                            const int* trig, int split, void* plan, void* grouped, void* slots, long slots_bytes,
                            void* work, long work_bytes, void* fit, hipStream_t stream) {
  if (batch < 1 || batch > kMaxFrames || max_n < 0 || point_step <= 0 || data_bytes < 0 ||
      data_bytes >= 0x80000000L || (n_stride != 1 && n_stride != 2) || (split != 0 && split != 1))
    return (int)hipErrorInvalidValue;
  if (max_clusters < 1 || max_clusters > kMaxClusters || angles < 2 || angles > kMaxAngles || d0q < 164 ||
      d0q > 16384)
    return (int)hipErrorInvalidValue;
  if (frame_off == nullptr || frame_n == nullptr || label == nullptr || table == nullptr || found == nullptr ||
      trig == nullptr || plan == nullptr || grouped == nullptr || slots == nullptr || work == nullptr ||
      fit == nullptr || (max_n > 0 && data == nullptr))
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)frame_off & 7) != 0 || ((uintptr_t)frame_n & 3) != 0 || ((uintptr_t)label & 3) != 0 ||
      ((uintptr_t)table & 7) != 0 || ((uintptr_t)found & 3) != 0 || ((uintptr_t)plan & 15) != 0 ||
      ((uintptr_t)grouped & 7) != 0 || ((uintptr_t)slots & 7) != 0 || ((uintptr_t)work & 3) != 0 ||
      ((uintptr_t)fit & 7) != 0)
    return (int)hipErrorInvalidValue;
  FitArgs a;
  a.step = point_step;
  a.off[0] = off_x; a.off[1] = off_y; a.off[2] = off_z; a.off[3] = -1;
  a.fast = cloud_fast_path(data, point_step, a.off, true);
  if (a.fast < 0) return (int)hipErrorInvalidValue;
  a.max_n = max_n; a.n_stride = n_stride; a.max_k = max_clusters; a.angles = angles; a.d0q = d0q; a.split = split;
  a.cap = max_n / kChunk + 1;
  a.records = (int)(data_bytes / point_step + 1);
  if (slots_bytes < (long)sizeof(Slot) * batch * a.cap * angles || work_bytes < 4L * batch * (2 + 5 * a.cap))
    return (int)hipErrorInvalidValue;  // a workspace shorter than the kernels index
  for (int j = 0; j < 2 * kMaxAngles; ++j) a.cs[j] = 0;
  for (int j = 0; j < angles; ++j) {
    const int c = trig[j], s = trig[angles + j];
    if (c < -16384 || c > 16384 || s < -16384 || s > 16384) return (int)hipErrorInvalidValue;
    a.cs[j] = c;
    a.cs[kMaxAngles + j] = s;
  }

  const uint8_t* in = (const uint8_t*)data;
  fit_plan_kernel<<<batch, kBlock, 0, stream>>>(data_bytes, frame_off, frame_n, (const Row*)table, (const int*)found,
                                                a, (Plan*)plan, (Slot*)slots, (int*)work, (FitRow*)fit);
  if (max_n > 0) {
    if (int e = (int)hipGetLastError()) return e;
    const dim3 pgrid((max_n + kBlock - 1) / kBlock, batch);
    fit_group_kernel<<<pgrid, kBlock, 0, stream>>>(in, data_bytes, frame_off, frame_n, (const int*)label,
                                                   (const Row*)table, (const int*)found, a, (Plan*)plan,
                                                   (int2*)grouped);
    if (int e = (int)hipGetLastError()) return e;
    fit_cluster_kernel<<<dim3(max_clusters, batch), kBlock, 0, stream>>>((const int*)found, a, (const Plan*)plan,
                                                                        (const int2*)grouped, (FitRow*)fit);
    if (split && max_n > kChunk) {
      if (int e = (int)hipGetLastError()) return e;
      const dim3 cgrid(2 * a.cap, batch);
      fit_chunk_bounds_kernel<<<cgrid, kBlock, 0, stream>>>(a, (const Plan*)plan, (const int2*)grouped,
                                                            (const int*)work, (Slot*)slots);
      if (int e = (int)hipGetLastError()) return e;
      fit_chunk_score_kernel<<<cgrid, kBlock, 0, stream>>>(a, (const Plan*)plan, (const int2*)grouped,
                                                           (const int*)work, (Slot*)slots);
      if (int e = (int)hipGetLastError()) return e;
      fit_select_kernel<<<dim3(a.cap, batch), kMaxAngles, 0, stream>>>(a, (const int*)work, (const Slot*)slots,
                                                                       (FitRow*)fit);
    }
  }
  TCA_LAUNCH_CHECK();
}
