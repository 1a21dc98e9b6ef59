// K37 — the inflation layer on K33's planes: per cell the cost of the squared distance, in cells, to the nearest
// occupied (100) cell of its own plane, by a host-built table (ops/occupancy_grid.py has the definition: integers
// only, so the bytes are equal, not near).  A bounded exact Euclidean distance transform, separable: the distance
// along the row to the nearest occupied cell, then the minimum over the rows of dy * dy + g * g.
//
// Batched over the B planes tca_occupancy_grid wrote: plane b at b * stride, stride = ceil(W * H / 16) * 16, W x H
// int8 cells, row-major.  The output has the same layout in a buffer of its own: a workgroup reads cells its
// neighbours write.  blockIdx.z = plane; one workgroup of 256 lanes (4 waves) owns a tile of 64 x 32 cells and walks
// the window of the tile plus a halo of R = radius_cells (<= 64) on every side: n = 32 + 2 R rows of 192 columns.
//
//   bits     a wave takes (row, 64-column word) pairs of the window, one lane per cell: a byte load (none for a
//            position outside the plane or further than R from the tile), __ballot(v == 100) is the word; lane 0
//            stores it: uint64 bits[n][3], 3,840 bytes at R = 64.  The tile's own bytes stay in LDS (own, 2 KiB).
//   empty    a wave that saw a set bit raises an LDS flag.  With no bit in the window every cell of the tile is
//            further than R from anything occupied: the tile's bytes are copied through (skip_empty = 1) and the
//            row and column passes and the table's load do not run.
//   rows     for every window row and tile column x the distance g to the nearest set bit of the row, from the
//            row's three words: the bits at or below x by __clzll, at or above by __ffsll, min of the two, 255 for
//            none within R: uint8 g[n][64], 10 KiB at R = 64.  A row without a bit is filled without looking.
//   columns  a lane owns four consecutive cells of a tile row (16 lanes per row, 4 rows per wave, two trips): one
//            LDS dword per window row holds its four g.  best = g * g of its own row, then dy = 1, 2, .. R both
//            ways, while dy * dy is below the largest of its four bests.  255 * 255 is above every R * R: "none"
//            needs no test of its own.  A wave's 64 dwords of one dy are 256 consecutive bytes: no bank is hit twice.
//   combine  table[d2] for d2 <= R * R (in LDS, at most 4,097 bytes), else 0; the value rule of the definition on
//            the cell's own byte; one 32-bit store of the four cells where they are inside the plane and their
//            address is 4-byte aligned (W % 4 == 0, or the row happens to be), bytewise otherwise.
//
// LDS is 24 n + 64 n + 2048 + table + 16 bytes: 19.8 KiB at R = 64, 5.7 KiB at R = 3.  No atomics, no workspace, no
// reset: a relaunch or a graph replay gives the same bytes.  No position outside a plane is read or written.
#include "tca_common.h"

using namespace tca;

namespace {

constexpr int kBlock = 256;
constexpr int kTileW = 64, kTileH = 32;
constexpr int kMaxRadius = 64;
constexpr int kMaxFrames = 64;    // the limits of tca_occupancy_grid (occupancy_grid.hip)
constexpr int kMaxSide = 2048;
constexpr int kMaxCells = 1 << 22;
constexpr int kMaxPlane = 1 << 24;
constexpr int kNone = 255;  // g of a row position without an occupied cell within R

struct InflateArgs {
  int W, H, R;
  int stride;   // cells from one plane to the next: a multiple of 16
  int unknown;  // inflate_unknown
  int skip;     // skip_empty
};

// The four results of cells whose own bytes are `own` (cell j in byte j) and squared distances d2[j].
__device__ __forceinline__ uint32_t combine4(uint32_t own, const int* d2, int r2, const uint8_t* lut, int unknown) {
  uint32_t packed = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int v = (int8_t)(own >> (8 * j));
    const int c = d2[j] <= r2 ? (int)lut[d2[j]] : 0;
    int res = v;  // 100 stays, and so does a byte that is none of the three values
    if (v == 0) res = c;
    else if (v == -1 && (unknown ? c > 0 : c >= 99)) res = c;
    packed |= ((uint32_t)res & 0xFFu) << (8 * j);
  }
  return packed;
}

__global__ void __launch_bounds__(kBlock) grid_inflate_kernel(const int8_t* __restrict__ planes,
                                                              const uint8_t* __restrict__ table, InflateArgs a,
                                                              int8_t* __restrict__ out) {
  extern __shared__ uint64_t lds[];
  const int R = a.R, n_rows = kTileH + 2 * R, r2 = R * R;
  uint64_t* bits = lds;                                         // [n_rows][3]
  uint8_t* g = reinterpret_cast<uint8_t*>(bits + 3 * n_rows);   // [n_rows][64]
  uint8_t* own = g + kTileW * n_rows;                           // [32][64]
  int* flag = reinterpret_cast<int*>(own + kTileW * kTileH);    // [4]: [0] a bit is set in the window
  uint8_t* lut = reinterpret_cast<uint8_t*>(flag + 4);          // [r2 + 1]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  const int8_t* plane = planes + (long)blockIdx.z * a.stride;
  int8_t* mine = out + (long)blockIdx.z * a.stride;

  if (tid == 0) flag[0] = 0;
  __syncthreads();

  // ------------------------------------------------------------------------------------ bits
  uint64_t seen = 0;
  for (int t = wave; t < 3 * n_rows; t += kBlock / 64) {  // (the same trips for every lane of a wave)
    const int r = t / 3, w = t - 3 * r;
    const int gy = y0 - R + r, px = (w - 1) * kTileW + lane, gx = x0 + px;  // px: the column against the tile's first
    int v = 0;
    if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W && px >= -R && px < kTileW + R) v = plane[(long)gy * a.W + gx];
    const uint64_t word = __ballot(v == 100);
    seen |= word;
    if (lane == 0) bits[t] = word;
    if (w == 1 && r >= R && r < R + kTileH) own[(r - R) * kTileW + lane] = (uint8_t)v;
  }
  if (seen != 0 && lane == 0) flag[0] = 1;  // (every writer stores the same value)
  __syncthreads();
  const bool empty = flag[0] == 0;  // the same for the whole workgroup

  if (!(empty && a.skip)) {
    for (int i = tid; i <= r2; i += kBlock) lut[i] = table[i];
    // ---------------------------------------------------------------------------------- rows
    for (int r = wave; r < n_rows; r += kBlock / 64) {
      const uint64_t w0 = bits[3 * r], w1 = bits[3 * r + 1], w2 = bits[3 * r + 2];
      int d = kNone;
      if ((w0 | w1 | w2) != 0) {
        const uint64_t below = w1 & (~0ull >> (63 - lane)), above = w1 >> lane;  // bits 0..lane, bits lane..63
        int dl = kNone, dr = kNone;
        if (below != 0) dl = lane - (63 - __clzll((long long)below));
        else if (w0 != 0) dl = lane + 1 + __clzll((long long)w0);
        if (above != 0) dr = __ffsll((unsigned long long)above) - 1;
        else if (w2 != 0) dr = kTileW - lane + __ffsll((unsigned long long)w2) - 1;
        d = min(dl, dr);
        if (d > R) d = kNone;
      }
      g[r * kTileW + lane] = (uint8_t)d;
    }
    __syncthreads();
  }

  // ------------------------------------------------------------------- columns and combine
  const int lx = 4 * (tid & 15);
  for (int y = tid >> 4; y < kTileH; y += kBlock / 16) {
    const int gx = x0 + lx, gy = y0 + y;
    if (gx >= a.W || gy >= a.H) continue;
    const uint32_t mine4 = *reinterpret_cast<const uint32_t*>(own + y * kTileW + lx);
    uint32_t packed = mine4;  // an empty window: every d2 is above r2, 0 stays 0 and -1 stays -1
    if (!(empty && a.skip)) {
      const int ry = R + y;
      int best[4];
      uint32_t q = *reinterpret_cast<const uint32_t*>(g + ry * kTileW + lx);
#pragma unroll
      for (int j = 0; j < 4; ++j) { const int d = (q >> (8 * j)) & 0xFF; best[j] = d * d; }
      for (int dy = 1; dy <= R; ++dy) {
        const int dy2 = dy * dy;
        if (dy2 >= max(max(best[0], best[1]), max(best[2], best[3]))) break;  // no row further away can be nearer
        const uint32_t up = *reinterpret_cast<const uint32_t*>(g + (ry - dy) * kTileW + lx);
        const uint32_t dn = *reinterpret_cast<const uint32_t*>(g + (ry + dy) * kTileW + lx);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int du = (up >> (8 * j)) & 0xFF, dd = (dn >> (8 * j)) & 0xFF, d = min(du, dd);
          best[j] = min(best[j], dy2 + d * d);
        }
      }
      packed = combine4(mine4, best, r2, lut, a.unknown);
    }
    const long at = (long)gy * a.W + gx;
    const int cnt = min(4, a.W - gx);
    // a plane starts 16-byte aligned in the output: the address is aligned iff the cell index is
    if (cnt == 4 && (at & 3) == 0) {
      *reinterpret_cast<uint32_t*>(mine + at) = packed;
    } else {
      for (int j = 0; j < cnt; ++j) mine[at + j] = (int8_t)(packed >> (8 * j));
    }
  }
}

}  // namespace

// planes: what tca_occupancy_grid wrote, int8, plane b's W * H cells at planes + b * stride with stride =
// ceil(W * H / 16) * 16; planes_bytes of it, at least (batch - 1) * stride + W * H.  radius_cells: R, 1..64.  lut:
// device uint8 [R * R + 1], the cost by squared distance in cells (ops/occupancy_grid.py's cost_table), lut_bytes of
// it.  inflate_unknown: 1, an unknown cell takes every cost above 0; 0, only 99 and 100 (costmap_2d's rule).
// skip_empty: 1, a tile with no occupied cell within R is copied through (0: measurements; the same bytes).  out: the
// same layout in another buffer, out_bytes of it; nothing in the padding or past (batch - 1) * stride + W * H is
// written.  Both buffers are 16-byte aligned and must not overlap.  What does not fit is refused before any launch.
TCA_API int tca_grid_inflate(const void* planes, long planes_bytes, int batch, int W, int H, int radius_cells,
                             const void* lut, long lut_bytes, int inflate_unknown, int skip_empty, void* out,
                             long out_bytes, hipStream_t stream) {
  if (batch < 1 || batch > kMaxFrames || W < 1 || W > kMaxSide || H < 1 || H > kMaxSide || (long)W * H > kMaxCells)
    return (int)hipErrorInvalidValue;
  if (radius_cells < 1 || radius_cells > kMaxRadius || lut_bytes < (long)radius_cells * radius_cells + 1)
    return (int)hipErrorInvalidValue;
  if ((inflate_unknown != 0 && inflate_unknown != 1) || (skip_empty != 0 && skip_empty != 1))
    return (int)hipErrorInvalidValue;
  const long stride = ((long)W * H + 15) / 16 * 16;
  const long extent = (batch - 1) * stride + (long)W * H;
  if ((long)batch * stride > kMaxPlane || planes_bytes < extent || out_bytes < extent)
    return (int)hipErrorInvalidValue;
  if (planes == nullptr || out == nullptr || lut == nullptr || ((uintptr_t)planes & 15) != 0 ||
      ((uintptr_t)out & 15) != 0)
    return (int)hipErrorInvalidValue;
  const uintptr_t in0 = (uintptr_t)planes, out0 = (uintptr_t)out;
  if (in0 < out0 + (uintptr_t)extent && out0 < in0 + (uintptr_t)extent) return (int)hipErrorInvalidValue;
  InflateArgs a;
  a.W = W; a.H = H; a.R = radius_cells; a.stride = (int)stride; a.unknown = inflate_unknown; a.skip = skip_empty;
  const int n_rows = kTileH + 2 * radius_cells;
  const size_t lds = (size_t)n_rows * (3 * sizeof(uint64_t) + kTileW) + kTileW * kTileH + 4 * sizeof(int) +
                     (size_t)radius_cells * radius_cells + 1;
  const dim3 grid((W + kTileW - 1) / kTileW, (H + kTileH - 1) / kTileH, batch);
  grid_inflate_kernel<<<grid, kBlock, lds, stream>>>((const int8_t*)planes, (const uint8_t*)lut, a, (int8_t*)out);
  TCA_LAUNCH_CHECK();
}
