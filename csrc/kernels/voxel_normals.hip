// K35 — a surface normal and a curvature per voxel of the thinned cloud: a fixed-radius neighbour search over cell
// lists and a batched 3x3 symmetric eigen-solve.  ops/voxel_downsample.py (normals_numpy) has the definition; these
// kernels give its bytes.  They run on the stream behind tca_voxel_downsample and read its records and counts[b] from
// the device: no host round trip lies between the two.
//
// Per voxel a: q = rint(c * 65536) of its published float32 centroid; its neighbours are the voxels b of the same
// cloud, itself included, with sum (q_b - q_a)^2 <= R^2 in int64 (a closed ball).  Ten integers are gathered about a:
// the count m, sum d (3) and sum d_i d_j (6).  R <= 4 leaves bounds the ball to 10^3 voxels and |d| to 2^18, so
// sum d < 2^28 (int32) and sum d d < 2^46 (int64).  Then C = Sdd - Sd Sd / m in float64, each entry rounded to
// float32, kSweeps cyclic Jacobi sweeps in float32, the column of the smallest diagonal entry renormalised and turned
// towards the origin, and max(l_min, 0) / (l0 + l1 + l2).  m < 3: four quiet NaNs.
//
// After the scatter of tca_voxel_downsample its leaf table (48 bytes a slot, slots[b] >= the cloud's points) is dead;
// its bytes are this launch's workspace: the cell lists of side R, which tca_cell_lists.h builds (reset, keys, starts,
// sort; K36's outlier filter builds the same).  (slot, rank) of the keys pass wait in the row's 16 bytes of the output,
// which the fit overwrites last.
//
//   fit     one lane per record in cell order, one wave per workgroup.  stage = 1: the wave loops over the distinct
//           cells among its lanes (a ballot, the first lane's cell broadcast); lanes 0..26 probe the 27 cells around it
//           — 27 probes per cell, not per row — a shuffle scan turns their counts into one run of candidates, which
//           goes through LDS 64 quads at a time, and the lanes of that cell gather their ten integers in registers.
//           stage = 0: every lane probes the 27 cells around its own and reads their quads from global memory.  Then
//           per lane the float64 covariance, the float32 Jacobi sweeps in registers and one 16-byte store at its row.
//
// The moments are integer sums, so neither the order of the cells nor the order inside a cell reaches an output byte.
// No workgroup waits on another, only integer atomics are used, the resets belong to the launch (a relaunch or a graph
// replay gives the same bytes), nothing is allocated and no hipMemset is used.  Contraction to FMA is switched off for
// this file; division and square root are IEEE.
#include "tca_cell_lists.h"

#include <cmath>

#pragma clang fp contract(off)

using namespace tca;

namespace {

constexpr int kSweeps = 4;  // ops/voxel_downsample.py SWEEPS
constexpr unsigned kNaN = 0x7FC00000u;

using NormalArgs = CellArgs;

struct Moments {
  int m, sd[3];
  long long sdd[6];  // xx, xy, xz, yy, yz, zz
};

__device__ __forceinline__ void gather(Moments& g, const int4& me, const int4& it, long long r2) {
  const int dx = it.x - me.x, dy = it.y - me.y, dz = it.z - me.z;  // |q| <= 2^25: no overflow
  const long long xx = (long long)dx * dx, yy = (long long)dy * dy, zz = (long long)dz * dz;
  if (xx + yy + zz > r2) return;
  g.m += 1;
  g.sd[0] += dx; g.sd[1] += dy; g.sd[2] += dz;
  g.sdd[0] += xx; g.sdd[1] += (long long)dx * dy; g.sdd[2] += (long long)dx * dz;
  g.sdd[3] += yy; g.sdd[4] += (long long)dy * dz; g.sdd[5] += zz;
}

// One Jacobi rotation of the pair (p, q), r the third index: docs/precision.md has this order of operations, and
// ops/voxel_downsample.py (_rotate) the same in NumPy.  An infinite theta gives t = 1 / inf = 0.
__device__ __forceinline__ void rotate(float& app, float& aqq, float& apq, float& arp, float& arq, float (&vp)[3],
                                       float (&vq)[3]) {
  if (apq == 0.f) return;
  const float theta = (aqq - app) / (apq + apq);
  const float t = (theta < 0.f ? -1.f : 1.f) / (fabsf(theta) + sqrtf(theta * theta + 1.f));
  const float c = 1.f / sqrtf(t * t + 1.f);
  const float s = t * c;
  const float h = t * apq;
  app = app - h;
  aqq = aqq + h;
  apq = 0.f;
  const float rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float p = vp[k], q = vq[k];
    vp[k] = c * p - s * q;
    vq[k] = s * p + c * q;
  }
}

__device__ __forceinline__ uint4 solve(const Moments& g, const float (&c)[3]) {
  if (g.m < 3) return make_uint4(kNaN, kNaN, kNaN, kNaN);
  const double fm = (double)g.m;
  const double d[3] = {(double)g.sd[0], (double)g.sd[1], (double)g.sd[2]};
  float a00 = (float)((double)g.sdd[0] - (d[0] * d[0]) / fm), a01 = (float)((double)g.sdd[1] - (d[0] * d[1]) / fm);
  float a02 = (float)((double)g.sdd[2] - (d[0] * d[2]) / fm), a11 = (float)((double)g.sdd[3] - (d[1] * d[1]) / fm);
  float a12 = (float)((double)g.sdd[4] - (d[1] * d[2]) / fm), a22 = (float)((double)g.sdd[5] - (d[2] * d[2]) / fm);
  float v0[3] = {1.f, 0.f, 0.f}, v1[3] = {0.f, 1.f, 0.f}, v2[3] = {0.f, 0.f, 1.f};  // the columns
#pragma unroll
  for (int sweep = 0; sweep < kSweeps; ++sweep) {
    rotate(a00, a11, a01, a02, a12, v0, v1);
    rotate(a00, a22, a02, a01, a12, v0, v2);
    rotate(a11, a22, a12, a01, a02, v1, v2);
  }
  int low = 0;
  float least = a00;
  if (a11 < least) { low = 1; least = a11; }
  if (a22 < least) { low = 2; least = a22; }
  float n[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) n[k] = low == 0 ? v0[k] : low == 1 ? v1[k] : v2[k];
  const float len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) n[k] = n[k] / len;
  const bool away = n[0] * c[0] + n[1] * c[1] + n[2] * c[2] > 0.f;
  const float total = a00 + a11 + a22;
  const float curv = total > 0.f ? (least < 0.f ? 0.f : least) / total : 0.f;
  return make_uint4(__float_as_uint(away ? -n[0] : n[0]), __float_as_uint(away ? -n[1] : n[1]),
                    __float_as_uint(away ? -n[2] : n[2]), __float_as_uint(curv));
}

template <bool kStage>
__global__ void __launch_bounds__(64) normals_fit_kernel(const uint4* __restrict__ rows, const int* __restrict__ counts,
                                                         NormalArgs a, const Cell* __restrict__ cells,
                                                         const int4* __restrict__ sorted, uint4* __restrict__ normals,
                                                         long n_records) {
  __shared__ int4 tile[64];
  const int b = blockIdx.y;
  const int K = records_of(counts, a, b);
  const long first = (long)blockIdx.x * 64;
  if (first >= K) return;  // the whole workgroup, one wave
  const int lane = threadIdx.x;
  const Cell* tab = cells + a.slot_off[b];
  const int4* srt = sorted + a.pt_off[b];
  const int mask = a.mask[b], R = a.radius;
  const long long r2 = (long long)R * R;

  bool active = first + lane < K;
  const int4 me = active ? srt[first + lane] : make_int4(0, 0, 0, -1);
  active = active && me.w >= 0 && me.w < K;
  const int cx = floor_div(me.x, R), cy = floor_div(me.y, R), cz = floor_div(me.z, R);
  Moments g = {};

  if (kStage) {
    unsigned long long todo = __ballot(active);
    while (todo) {  // (the same trips for every lane: one wave)
      const int lead = __ffsll((long long)todo) - 1;
      const int lx = __shfl(cx, lead, 64), ly = __shfl(cy, lead, 64), lz = __shfl(cz, lead, 64);
      const bool mine = active && cx == lx && cy == ly && cz == lz;
      todo &= ~__ballot(mine);
      int start = 0, count = 0;
      if (lane < 27) count = find_cell(tab, mask, cell_key(lx + lane % 3 - 1, ly + lane / 3 % 3 - 1, lz + lane / 9 - 1), K, &start);
      int upto = count;
#pragma unroll
      for (int o = 1; o < 32; o <<= 1) {
        const int t = __shfl_up(upto, o, 64);
        if (lane >= o) upto += t;
      }
      const int total = __shfl(upto, 26, 64);
      const int before = upto - count;
      for (int t0 = 0; t0 < total; t0 += 64) {
        const int e = t0 + lane;
        int src = -1;
        for (int k = 0; k < 27; ++k) {
          const int pk = __shfl(before, k, 64), nk = __shfl(count, k, 64), sk = __shfl(start, k, 64);
          if (e >= pk && e < pk + nk) src = sk + (e - pk);
        }
        __syncthreads();  // the tile's readers of the last trip
        if (src >= 0 && src < K) tile[lane] = srt[src];
        __syncthreads();
        const int here = min(64, total - t0);
        if (mine)
          for (int k = 0; k < here; ++k) gather(g, me, tile[k], r2);
      }
    }
  } else if (active) {
    for (int k = 0; k < 27; ++k) {
      int start = 0;
      const int count = find_cell(tab, mask, cell_key(cx + k % 3 - 1, cy + k / 3 % 3 - 1, cz + k / 9 - 1), K, &start);
      for (int e = 0; e < count; ++e) gather(g, me, srt[start + e], r2);
    }
  }
  if (!active) return;
  const uint4 rec = rows[a.pt_off[b] + me.w];
  const float c[3] = {__uint_as_float(rec.x), __uint_as_float(rec.y), __uint_as_float(rec.z)};
  const long to = (long)a.pt_off[b] + me.w;
  if (to < n_records) normals[to] = solve(g, c);
}

}  // namespace

// rows: the 16-byte records tca_voxel_downsample wrote (device, 16-byte aligned, rows_bytes >= 16 * sum(ns)), cloud
// b's from record sum(ns[:b]); counts int[B] (device): the records of every cloud, clamped to ns[b].  ns, slots: HOST
// int[B], what tca_voxel_downsample took.  radius_q: the ball's radius in units of 2^-16 m, 1..4 * 65536.  stage: 0,
// every lane probes and reads for itself (what runs: profiles/voxel_normals/README.md); 1: the candidates of a cell's
// 27 neighbours go through LDS once per cell.  table: the leaf table's bytes (48 * sum(slots), 16-byte aligned), reset here on the stream;
// normals: 16 bytes per record at the record's index (normal x, y, z, curvature), normals_bytes >= 16 * sum(ns),
// 16-byte aligned; only the first counts[b] of a cloud are written.  A buffer shorter than that, or misaligned, is
// refused, and nothing is launched.
TCA_API int tca_voxel_normals(const void* rows, long rows_bytes, const int* counts, const int* ns, const int* slots,
                              int batch, int radius_q, int stage, void* table, long table_bytes, void* normals,
                              long normals_bytes, hipStream_t stream) {
  CellPlan p;
  if ((stage != 0 && stage != 1) || !cell_plan(ns, slots, batch, radius_q, 0, table, table_bytes, p))
    return (int)hipErrorInvalidValue;
  if (rows_bytes < 16 * p.n_sum || normals_bytes < 16 * p.n_sum) return (int)hipErrorInvalidValue;
  if (rows == nullptr || counts == nullptr || normals == nullptr) return (int)hipErrorInvalidValue;
  if (((uintptr_t)rows & 15) != 0 || ((uintptr_t)normals & 15) != 0 || ((uintptr_t)counts & 3) != 0)
    return (int)hipErrorInvalidValue;
  if (p.a.max_n == 0) return (int)hipSuccess;

  const uint4* in = (const uint4*)rows;
  uint4* out = (uint4*)normals;
  if (int e = cell_lists_build(p, in, counts, batch, 0, out, stream)) return e;
  const dim3 grid((p.a.max_n + 63) / 64, batch);
  if (stage)
    normals_fit_kernel<true><<<grid, 64, 0, stream>>>(in, counts, p.a, p.cells, p.sorted, out, p.n_sum);
  else
    normals_fit_kernel<false><<<grid, 64, 0, stream>>>(in, counts, p.a, p.cells, p.sorted, out, p.n_sum);
  TCA_LAUNCH_CHECK();
}
