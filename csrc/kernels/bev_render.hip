// K23 — the bird's-eye-view picture of a batch of LiDAR frames and their detections, pixel for
// pixel the host painter's (utils/bev.py render_bev_frame, the definition).
//
// Batched over B frames that share one view and one record layout.  Three kernels on the stream,
// after the level plane is zeroed there (the plane is workspace, not output):
//
//  * points: one lane per point, blocks of 256.  Raw PointCloud2 bytes are read in place as in
//    K22 (per-frame byte offset + point count in device arrays; a 16-byte, a dword or a byte load
//    path, chosen per frame from the alignment).  Record mode (an intensity offset >= 0) is
//    cloud_to_numpy(z_offset = zo) followed by level_plane: a point with a NaN in x, y, z or
//    intensity is dropped, z' = z + zo.  Dense mode (intensity offset -1) reads fp32 rows whose z
//    already carries zo, and has no NaN-row rule.  Then the painter's rule, every fp32 operation
//    rounded on its own (contraction to FMA is switched off for this file):
//        fr = (x1 - x) * inv, fc = (y1 - y) * inv; kept iff 0 <= fr < H, 0 <= fc < W, z' finite
//        t = ((z' - zo) - z0) * zscale; level = 55 + (t >= 200 ? 200 : t > 0 ? floor(t) : 0)
//    The six constants come from the host (BevView.constants() and float32(zo)).
//    A pixel takes the maximum level of its points.  There is no byte atomicMax, so the plane
//    packs four pixels of a row into one 32-bit word (rows padded to whole words): a lane reads
//    the word, leaves if the stored byte is already >= its level, and otherwise swaps in the word
//    with its byte raised (atomicCAS), retrying on the returned word.  Bytes only grow, so a stale
//    read can only cause a CAS that fails and retries, never a wrong skip, and the loop ends
//    after at most the 4 x 201 raises a word can take.  The early skip is what keeps contention
//    low: a LiDAR ring puts runs of consecutive points on one pixel, and once the pixel holds
//    level L only a higher point issues an atomic at all.  The maximum of integers does not
//    depend on arrival order.
//  * compose: plane -> (level, level, level) in out (uint8 [B, H, W, 3], rows row_stride bytes
//    apart).  Consecutive lanes write consecutive bytes of a row: one dword store per lane over
//    the 4-byte aligned middle of the row, wherever its base lies, and byte stores for the up to
//    three bytes before and after it.  Bytes of a row past 3 * W are not written.
//  * boxes and labels: one workgroup per frame, structured like K15's draw_kernel.  Boxes in
//    order with a barrier between them (a later box wins); per box edges 1, 2, 3 in the label
//    colour, a barrier, edge 0 in the heading colour.  The line rule is edge_pixels: ends in
//    lexicographic order, n = max(|dx|, |dy|), sample i of 0..n at a + floor((2 i d + n) / 2n) per
//    coordinate (a floor division, in 64 bits: corners are clamped to +-32768, so 2 i d reaches
//    8.6e9).  Pixels outside the image are dropped.  Then the labels in order, 6x11 glyphs of
//    tca_font6x11.h at (min corner col + 2, max(min corner row - 11, 0)), clipped on all four
//    sides.
//
// The box table is made on the host (ops/bev.py bev_box_table), since the definition takes
// NumPy's fp32 cos / sin, which no device routine is bound to reproduce: 12 ints per box,
//   0..7 corner (col, row) x 4, 8 valid (0: a NaN corner, not drawn), 9 colour r | g << 8 | b << 16,
//   10, 11 byte offset and length of its label in the text buffer (length 0: no label).
// No transcendental and no text formatting runs here.
#include "tca_common.h"
#include "tca_font6x11.h"

#pragma clang fp contract(off)

using namespace tca;

namespace {

constexpr int kBlock = 256;
constexpr int kDrawBlock = 1024;
constexpr int kRow = 12;  // ints per box table row
constexpr uint32_t kHeading = 255u | (80u << 8) | (40u << 16);

struct BevLayout {
  int step;
  int off[4];  // byte offset of x, y, z, intensity in a record; intensity -1: dense mode
  // 2: x, y, z are the dwords at 0 / 4 / 8 (intensity at 12 or absent), step % 16 == 0 and the base pointer is
  //    16-B aligned (one 16-B load per point); 1: offsets, step and base pointer are 4-B aligned (dword loads);
  // 0: byte loads.  The frame's byte offset must be as aligned, checked per block.
  int fast;
};

struct BevConst {
  float x1, y1, inv, z0, zscale, zo;
};

__device__ __forceinline__ uint32_t load_u32_bytes(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

__global__ void __launch_bounds__(kBlock) bev_points_kernel(
    const uint8_t* __restrict__ data, long data_bytes, const long* __restrict__ frame_off,
    const int* __restrict__ frame_n, BevLayout lay, BevConst k, int H, int W, int pw, uint32_t* __restrict__ plane) {
  const int b = blockIdx.y;
  const int n = frame_n[b];
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const long foff = frame_off[b];
  const long at = foff + i * lay.step;
  if (foff < 0 || at + lay.step > data_bytes) return;  // a record outside the buffer is not read
  const int fast = (lay.fast == 2 && (foff & 15) == 0) ? 2 : (lay.fast >= 1 && (foff & 3) == 0) ? 1 : 0;
  const bool record = lay.off[3] >= 0;

  uint32_t raw[4] = {0u, 0u, 0u, 0u};
  const uint8_t* rec = data + at;
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
  const float x = __uint_as_float(raw[0]), y = __uint_as_float(raw[1]);
  float z = __uint_as_float(raw[2]);
  if (record) {
    const float in = __uint_as_float(raw[3]);
    if (x != x || y != y || z != z || in != in) return;  // cloud_to_numpy(skip_nans)
    z = z + k.zo;
  }
  const float fr = (k.x1 - x) * k.inv;
  const float fc = (k.y1 - y) * k.inv;
  if (!(fr >= 0.f && fr < (float)H && fc >= 0.f && fc < (float)W && fabsf(z) <= 3.402823466e+38f)) return;
  const float t = ((z - k.zo) - k.z0) * k.zscale;
  const float lf = t >= 200.f ? 200.f : (t > 0.f ? floorf(t) : 0.f);
  const uint32_t lv = 55u + (uint32_t)(int)lf;
  const int r = (int)fr, c = (int)fc;  // 0 <= fr < H: truncation is the floor
  uint32_t* w = plane + ((long)b * H + r) * pw + (c >> 2);
  const int sh = 8 * (c & 3);
  uint32_t cur = *w;
  while (((cur >> sh) & 255u) < lv) {
    const uint32_t seen = atomicCAS(w, cur, (cur & ~(255u << sh)) | (lv << sh));
    if (seen == cur) break;
    cur = seen;
  }
}

// grid (blocks over a row's lanes, H, B).  A row's 3W bytes are `head` bytes up to its first 4-byte boundary (the
// row base need not be aligned), `full` whole dwords and a tail: lane j < full stores the dword at head + 4j, lane
// `full` stores the head and tail bytes one by one.
__global__ void __launch_bounds__(kBlock) bev_compose_kernel(const uint8_t* __restrict__ plane, int H, int W, int pw,
                                                             uint8_t* __restrict__ out, long frame_stride,
                                                             int row_stride) {
  const int b = blockIdx.z, r = blockIdx.y;
  const int j = blockIdx.x * kBlock + threadIdx.x;
  const uint8_t* src = plane + ((long)b * H + r) * pw * 4;
  uint8_t* dst = out + (long)b * frame_stride + (long)r * row_stride;
  const int nbytes = 3 * W;
  const int head = min((int)((4 - ((uintptr_t)dst & 3)) & 3), nbytes);
  const int full = (nbytes - head) >> 2;
  if (j < full) {
    const int o = head + 4 * j;
    const int p = o / 3, ph = o - 3 * p;  // bytes o .. o + 3 (< 3W) lie in pixels p and p + 1 (< W)
    const uint32_t a = src[p], c = src[p + 1];
    // ph 0: a a a c; 1: a a c c; 2: a c c c
    const uint32_t v = a | ((ph == 2 ? c : a) << 8) | ((ph == 0 ? a : c) << 16) | (c << 24);
    *reinterpret_cast<uint32_t*>(dst + o) = v;
  } else if (j == full) {
    for (int q = 0; q < head; ++q) dst[q] = src[q / 3];
    for (int q = head + 4 * full; q < nbytes; ++q) dst[q] = src[q / 3];
  }
}

__device__ __forceinline__ void put_px(uint8_t* f, int row_stride, int H, int W, long x, long y, uint32_t col) {
  if (x < 0 || x >= W || y < 0 || y >= H) return;
  uint8_t* p = f + y * row_stride + x * 3;
  p[0] = (uint8_t)(col & 255u);
  p[1] = (uint8_t)((col >> 8) & 255u);
  p[2] = (uint8_t)((col >> 16) & 255u);
}

__device__ __forceinline__ long floor_div(long a, long d) {  // d > 0
  long q = a / d;
  return (a % d != 0 && a < 0) ? q - 1 : q;
}

// edge_pixels of (ax, ay) - (bx, by), the whole workgroup striding over the samples
__device__ void draw_edge(uint8_t* f, int row_stride, int H, int W, int ax, int ay, int bx, int by, uint32_t col) {
  if (bx < ax || (bx == ax && by < ay)) {
    int t = ax; ax = bx; bx = t;
    t = ay; ay = by; by = t;
  }
  const long dx = (long)bx - ax, dy = (long)by - ay;
  const long n = max(dx < 0 ? -dx : dx, dy < 0 ? -dy : dy);
  if (n == 0) {
    if (threadIdx.x == 0) put_px(f, row_stride, H, W, ax, ay, col);
    return;
  }
  for (long i = threadIdx.x; i <= n; i += blockDim.x)
    put_px(f, row_stride, H, W, ax + floor_div(2 * i * dx + n, 2 * n), ay + floor_div(2 * i * dy + n, 2 * n), col);
}

__global__ void __launch_bounds__(kDrawBlock) bev_boxes_kernel(uint8_t* __restrict__ out, long frame_stride, int H,
                                                               int W, int row_stride, const int* __restrict__ box_off,
                                                               const int* __restrict__ table, int n_boxes,
                                                               const uint8_t* __restrict__ text, int text_bytes) {
  const int b = blockIdx.x;
  uint8_t* f = out + (long)b * frame_stride;
  const int k0 = max(box_off[b], 0), k1 = min(box_off[b + 1], n_boxes);  // block-uniform
  for (int k = k0; k < k1; ++k) {
    const int* t = table + (long)k * kRow;
    if (t[8] != 0) {
      const uint32_t col = (uint32_t)t[9];
#pragma unroll
      for (int e = 1; e < 4; ++e) {
        const int g = (e + 1) & 3;
        draw_edge(f, row_stride, H, W, t[2 * e], t[2 * e + 1], t[2 * g], t[2 * g + 1], col);
      }
      __syncthreads();  // the heading side goes on top of its own box
      draw_edge(f, row_stride, H, W, t[0], t[1], t[2], t[3], kHeading);
    }
    __syncthreads();  // the next box overwrites this one where they overlap
  }
  for (int k = k0; k < k1; ++k) {
    const int* t = table + (long)k * kRow;
    const int to = t[10], L = t[11];
    if (t[8] == 0 || L <= 0 || to < 0 || (long)to + L > text_bytes) continue;  // block-uniform
    const uint32_t col = (uint32_t)t[9];
    const int x0 = min(min(t[0], t[2]), min(t[4], t[6])) + 2;
    const int y0 = max(min(min(t[1], t[3]), min(t[5], t[7])) - TCA_FONT_H, 0);
    const int cols = L * TCA_FONT_W, total = cols * TCA_FONT_H;
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
      const int row = i / cols, cx = i % cols;
      int ch = text[to + cx / TCA_FONT_W];
      ch = (ch < TCA_FONT_FIRST || ch > TCA_FONT_LAST) ? '?' : ch;
      if ((tca_font6x11[ch - TCA_FONT_FIRST][row] >> (cx % TCA_FONT_W)) & 1)
        put_px(f, row_stride, H, W, (long)x0 + cx, (long)y0 + row, col);
    }
    __syncthreads();  // later labels win
  }
}

}  // namespace

// data: device bytes, data_bytes of them (no record outside is read); frame_off long[B] (bytes) / frame_n int[B]:
// device; max_n: the largest frame_n (host, sizes the grid); offsets of x, y, z, intensity in a record of FLOAT32
// fields, intensity -1: dense mode (fp32 rows whose z carries zo, no NaN-row rule).  x1, y1, inv, z0, zscale:
// BevView.constants(); zo: float32(z_offset).  plane: B * H * ((W + 3) / 4) ints of workspace, zeroed here on the
// stream.  box_off int[B + 1], table int[n_boxes, 12], text uint8[text_bytes]: device.  out: uint8 [B, H, W, 3],
// rows row_stride >= 3 * W bytes apart, frames frame_stride >= H * row_stride bytes apart.
TCA_API int tca_bev_render(const void* data, long data_bytes, const long* frame_off, const int* frame_n, int batch,
                           int max_n, int point_step, int off_x, int off_y, int off_z, int off_i, float x1, float y1,
                           float inv, float z0, float zscale, float zo, int H, int W, int* plane, const int* box_off,
                           const int* table, int n_boxes, const void* text, int text_bytes, void* out,
                           long frame_stride, int row_stride, hipStream_t stream) {
  if (batch < 0 || batch > 65535 || max_n < 0 || n_boxes < 0 || text_bytes < 0 || data_bytes < 0 || point_step <= 0)
    return (int)hipErrorInvalidValue;
  if (H < 1 || H > 32767 || W < 1 || W > 32767 || row_stride < 3 * W || frame_stride < (long)H * row_stride)
    return (int)hipErrorInvalidValue;
  BevLayout lay;
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
             : (off_x == 0 && off_y == 4 && off_z == 8 && (off_i == 12 || off_i == -1) && (point_step & 15) == 0 &&
                ((uintptr_t)data & 15) == 0) ? 2 : 1;
  if (batch == 0) return 0;
  const int pw = (W + 3) / 4;
  const long words = (long)batch * H * pw;
  if (words > 0x7fffffffL || out == nullptr || plane == nullptr || frame_off == nullptr || frame_n == nullptr ||
      box_off == nullptr || (max_n > 0 && data == nullptr) || (n_boxes > 0 && table == nullptr) ||
      (text_bytes > 0 && text == nullptr))
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)plane & 3) != 0 || ((uintptr_t)frame_n & 3) != 0 || ((uintptr_t)box_off & 3) != 0 ||
      ((uintptr_t)table & 3) != 0 || ((uintptr_t)frame_off & 7) != 0)
    return (int)hipErrorInvalidValue;
  if (int e = zero_i32_async(plane, (int)words, stream)) return e;
  if (max_n > 0) {
    const BevConst k = {x1, y1, inv, z0, zscale, zo};
    dim3 grid((max_n + kBlock - 1) / kBlock, batch);
    bev_points_kernel<<<grid, kBlock, 0, stream>>>((const uint8_t*)data, data_bytes, frame_off, frame_n, lay, k, H, W,
                                                   pw, (uint32_t*)plane);
    if (int e = (int)hipGetLastError()) return e;
  }
  const int lanes = (3 * W) / 4 + 1;
  dim3 cgrid((lanes + kBlock - 1) / kBlock, H, batch);
  bev_compose_kernel<<<cgrid, kBlock, 0, stream>>>((const uint8_t*)plane, H, W, pw, (uint8_t*)out, frame_stride,
                                                   row_stride);
  if (int e = (int)hipGetLastError()) return e;
  if (n_boxes > 0)
    bev_boxes_kernel<<<batch, kDrawBlock, 0, stream>>>((uint8_t*)out, frame_stride, H, W, row_stride, box_off, table,
                                                       n_boxes, (const uint8_t*)text, text_bytes);
  TCA_LAUNCH_CHECK();
}
