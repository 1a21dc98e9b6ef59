// Raw sensor_msgs/Image payloads -> packed rgb8 on the device: the twelve encodings of
// ops/golden.py IMAGE_ENCODINGS, byte for byte what golden.image_to_rgb8 returns (that
// function is the specification; docs/precision.md "Raw Image encodings").
//
// A pure bandwidth kernel.  One thread makes four adjacent pixels of one row (12 output
// bytes: three dword stores where the destination is dword-aligned) from the 4 * bpp source
// bytes under them; a row whose width is no multiple of four ends in a per-pixel tail.  The
// row pitch `step` is arbitrary, so a row may start at any address: a run of source bytes is
// read with dword / 8-B / 16-B loads only where its address is aligned to that width, else
// byte by byte.  Every load, wide or not, covers only bytes of the packed row the thread's
// own pixels (and, for Bayer, their reflected neighbours) occupy, so nothing at or beyond
// (H-1)*step + packed_row of a frame is ever read: the last row's padding need not exist.
//
// One kernel instantiation per encoding (class x its compile-time parameters): the code is
// resolved by the launcher, never per pixel.
#include "tca_common.h"

namespace {

constexpr int kPx = 4;         // pixels per thread
constexpr int kThreads = 256;

struct Geo {
  const uint8_t* src;
  uint8_t* dst;
  int sfs, dfs;  // frame strides in bytes
  int step, H, W, n;
};

__device__ __forceinline__ int clip8(int v) { return min(max(v, 0), 255); }

// N source bytes (N in 4, 8, 12, 16) at p into dwords, little endian, with the widest loads
// p's alignment allows.
template <int N> __device__ __forceinline__ void load_run(const uint8_t* p, uint32_t (&w)[N / 4]) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if constexpr (N == 16) {
    if ((a & 15) == 0) {
      const uint4 v = *reinterpret_cast<const uint4*>(p);
      w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
      return;
    }
  }
  if constexpr (N == 8) {
    if ((a & 7) == 0) {
      const uint2 v = *reinterpret_cast<const uint2*>(p);
      w[0] = v.x, w[1] = v.y;
      return;
    }
  }
  if ((a & 3) == 0) {
#pragma unroll
    for (int i = 0; i < N / 4; ++i) w[i] = reinterpret_cast<const uint32_t*>(p)[i];
  } else {
#pragma unroll
    for (int i = 0; i < N / 4; ++i)
      w[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 |
             (uint32_t)p[4 * i + 3] << 24;
  }
}

// byte i of a run loaded by load_run (i is a constant after unrolling)
template <int NW> __device__ __forceinline__ int byte_of(const uint32_t (&w)[NW], int i) {
  return (int)((w[i >> 2] >> (8 * (i & 3))) & 0xffu);
}

// the 12 bytes of four rgb pixels
__device__ __forceinline__ void store_quad(uint8_t* p, const int (&o)[3 * kPx]) {
  if ((reinterpret_cast<uintptr_t>(p) & 3) == 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
      reinterpret_cast<uint32_t*>(p)[i] = (uint32_t)o[4 * i] | (uint32_t)o[4 * i + 1] << 8 |
                                          (uint32_t)o[4 * i + 2] << 16 | (uint32_t)o[4 * i + 3] << 24;
  } else {
#pragma unroll
    for (int i = 0; i < 3 * kPx; ++i) p[i] = (uint8_t)o[i];
  }
}

// ---- byte permutations: rgb8 (padded rows) / bgr8 / rgba8 / bgra8
template <int BPP, bool SWAP> struct Perm {
  static __device__ __forceinline__ void quad(const uint8_t* s, const Geo& g, int y, int x, int (&o)[3 * kPx]) {
    uint32_t w[BPP];
    load_run<4 * BPP>(s + y * g.step + x * BPP, w);
#pragma unroll
    for (int i = 0; i < kPx; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) o[3 * i + c] = byte_of(w, BPP * i + (SWAP ? 2 - c : c));
  }
  static __device__ __forceinline__ void pixel(const uint8_t* s, const Geo& g, int y, int x, int (&o)[3]) {
    const uint8_t* p = s + y * g.step + x * BPP;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = p[SWAP ? 2 - c : c];
  }
};

// ---- mono8 / mono16 ((v + 128) / 257, v assembled by the message's endianness)
template <int BYTES, bool BE> struct Mono {
  static __device__ __forceinline__ int gray(int b0, int b1) {
    const int v = BE ? (b0 << 8 | b1) : (b1 << 8 | b0);
    return (v + 128) / 257;
  }
  static __device__ __forceinline__ void quad(const uint8_t* s, const Geo& g, int y, int x, int (&o)[3 * kPx]) {
    uint32_t w[BYTES];
    load_run<4 * BYTES>(s + y * g.step + x * BYTES, w);
#pragma unroll
    for (int i = 0; i < kPx; ++i) {
      const int v = BYTES == 1 ? byte_of(w, i) : gray(byte_of(w, 2 * i), byte_of(w, 2 * i + 1));
      o[3 * i] = o[3 * i + 1] = o[3 * i + 2] = v;
    }
  }
  static __device__ __forceinline__ void pixel(const uint8_t* s, const Geo& g, int y, int x, int (&o)[3]) {
    const uint8_t* p = s + y * g.step + x * BYTES;
    o[0] = o[1] = o[2] = BYTES == 1 ? (int)p[0] : gray(p[0], p[1]);
  }
};

// ---- YUV 4:2:2 (UYVY / YUY2): BT.601 limited range, 20-bit fixed point, all in int32
// (|value| < 3.3e8); the shift is arithmetic on a possibly negative sum, then the clip
__device__ __forceinline__ void yuv_rgb(int y, int u, int v, int* o) {
  constexpr int kShift = 20, kCY = 1220542, kCVR = 1673527, kCVG = -852492, kCUG = -409993, kCUB = 2116026;
  u -= 128, v -= 128;
  const int yy = max(y - 16, 0) * kCY + (1 << (kShift - 1));
  o[0] = clip8((yy + kCVR * v) >> kShift);
  o[1] = clip8((yy + kCVG * v + kCUG * u) >> kShift);
  o[2] = clip8((yy + kCUB * u) >> kShift);
}

template <bool YUY2> struct Yuv {
  // a thread owns whole macropixels (4 bytes, 2 pixels): two per quad
  static __device__ __forceinline__ void quad(const uint8_t* s, const Geo& g, int y, int x, int (&o)[3 * kPx]) {
    uint32_t w[2];
    load_run<8>(s + y * g.step + x * 2, w);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int b0 = byte_of(w, 4 * m), b1 = byte_of(w, 4 * m + 1), b2 = byte_of(w, 4 * m + 2),
                b3 = byte_of(w, 4 * m + 3);
      const int u = YUY2 ? b1 : b0, v = YUY2 ? b3 : b2;
      yuv_rgb(YUY2 ? b0 : b1, u, v, &o[6 * m]);
      yuv_rgb(YUY2 ? b2 : b3, u, v, &o[6 * m + 3]);
    }
  }
  static __device__ __forceinline__ void pixel(const uint8_t* s, const Geo& g, int y, int x, int (&o)[3]) {
    const uint8_t* p = s + y * g.step + (x >> 1) * 4;
    const int u = p[YUY2 ? 1 : 0], v = p[YUY2 ? 3 : 2];
    const int lum = p[(YUY2 ? 0 : 1) + 2 * (x & 1)];
    yuv_rgb(lum, u, v, o);
  }
};

// ---- 8-bit Bayer, bilinear on the colour-filter plane extended by reflect-101 (row -1 is
// row 1, row H is row H-2, the same for columns).  (RY, RX): the red site of the 2x2 tile.
template <int RY, int RX> struct Bayer {
  // colour of a site from its centre and neighbour sums; red_col / red_row: the site's
  // column / row holds red samples
  static __device__ __forceinline__ void site(bool red_row, bool red_col, int c, int n, int s, int w, int e,
                                              int nw, int ne, int sw, int se, int* o) {
    const int cross = (n + s + w + e + 2) >> 2, diag = (nw + ne + sw + se + 2) >> 2;
    const int horiz = (w + e + 1) >> 1, vert = (n + s + 1) >> 1;
    if (red_col) {  // red site, or the green site of a blue row
      o[0] = red_row ? c : vert;
      o[1] = red_row ? cross : c;
      o[2] = red_row ? diag : horiz;
    } else {        // the green site of a red row, or a blue site
      o[0] = red_row ? horiz : diag;
      o[1] = red_row ? c : cross;
      o[2] = red_row ? vert : c;
    }
  }
  // x is a multiple of 4, so the column parity of pixel i is a compile-time value per lane
  static __device__ __forceinline__ void quad(const uint8_t* s, const Geo& g, int y, int x, int (&o)[3 * kPx]) {
    const int ys[3] = {y == 0 ? 1 : y - 1, y, y == g.H - 1 ? g.H - 2 : y + 1};
    const int xl = x == 0 ? 1 : x - 1, xr = x + kPx == g.W ? g.W - 2 : x + kPx;
    int t[3][kPx + 2];  // columns x-1 .. x+4 of rows y-1 .. y+1, reflected
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint8_t* row = s + ys[k] * g.step;
      uint32_t w[1];
      load_run<4>(row + x, w);
      t[k][0] = row[xl];
#pragma unroll
      for (int i = 0; i < kPx; ++i) t[k][i + 1] = byte_of(w, i);
      t[k][kPx + 1] = row[xr];
    }
    const bool red_row = ((y ^ RY) & 1) == 0;
#pragma unroll
    for (int i = 0; i < kPx; ++i)
      site(red_row, ((i ^ RX) & 1) == 0, t[1][i + 1], t[0][i + 1], t[2][i + 1], t[1][i], t[1][i + 2], t[0][i],
           t[0][i + 2], t[2][i], t[2][i + 2], &o[3 * i]);
  }
  static __device__ __forceinline__ void pixel(const uint8_t* s, const Geo& g, int y, int x, int (&o)[3]) {
    const uint8_t* r0 = s + (y == 0 ? 1 : y - 1) * g.step;
    const uint8_t* r1 = s + y * g.step;
    const uint8_t* r2 = s + (y == g.H - 1 ? g.H - 2 : y + 1) * g.step;
    const int xl = x == 0 ? 1 : x - 1, xr = x == g.W - 1 ? g.W - 2 : x + 1;
    site(((y ^ RY) & 1) == 0, ((x ^ RX) & 1) == 0, r1[x], r0[x], r2[x], r1[xl], r1[xr], r0[xl], r0[xr], r2[xl],
         r2[xr], o);
  }
};

// idx: a quad of a frame in row-major order (adjacent lanes: adjacent quads); blockIdx.y
// strides over the frames.  32-bit index math: the launcher bounds n * frame stride.
template <class E> __global__ void __launch_bounds__(kThreads) image_to_rgb8_kernel(Geo g, int qpr, int total) {
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const int y = idx / qpr, x = (idx - y * qpr) * kPx;
  for (int f = blockIdx.y; f < g.n; f += gridDim.y) {
    const uint8_t* s = g.src + f * g.sfs;
    uint8_t* d = g.dst + f * g.dfs + (y * g.W + x) * 3;
    if (x + kPx <= g.W) {
      int o[3 * kPx];
      E::quad(s, g, y, x, o);
      store_quad(d, o);
    } else {  // the row's ragged tail, per pixel
      for (int px = x; px < g.W; ++px, d += 3) {
        int o[3];
        E::pixel(s, g, y, px, o);
        d[0] = (uint8_t)o[0], d[1] = (uint8_t)o[1], d[2] = (uint8_t)o[2];
      }
    }
  }
}

template <class E> int launch(const Geo& g, hipStream_t stream) {
  const int qpr = (g.W + kPx - 1) / kPx;
  const int total = g.H * qpr;
  const dim3 grid((total + kThreads - 1) / kThreads, g.n < 65535 ? g.n : 65535);
  image_to_rgb8_kernel<E><<<grid, kThreads, 0, stream>>>(g, qpr, total);
  TCA_LAUNCH_CHECK();
}

}  // namespace

// n frames of one encoding and geometry: src rows of pitch `step` bytes, frame f at
// src + f * src_frame_stride; dst packed [n, H, W, 3] uint8, frame f at dst + f * dst_frame_stride.
// code: ops/golden.py IMAGE_ENCODINGS.  is_bigendian matters for mono16 only.  Nonzero (and no
// launch) for an unknown code, a step below the packed row, an odd-width YUV image, a Bayer
// image under 2x2, frame strides below a frame, or n * max(stride) >= 2^31.
TCA_API int tca_image_to_rgb8(const void* src, long src_frame_stride, int step, int H, int W, int code,
                              int is_bigendian, void* dst, long dst_frame_stride, int n, hipStream_t stream) {
  static const int kBpp[12] = {3, 3, 4, 4, 1, 2, 2, 2, 1, 1, 1, 1};
  if (code < 0 || code > 11 || n < 0 || H < 1 || W < 1) return (int)hipErrorInvalidValue;
  const long packed = (long)W * kBpp[code];
  if (step < packed) return (int)hipErrorInvalidValue;
  if ((code == 6 || code == 7) && (W & 1)) return (int)hipErrorInvalidValue;
  if (code >= 8 && (H < 2 || W < 2)) return (int)hipErrorInvalidValue;
  const long need = (long)(H - 1) * step + packed, frame = (long)H * W * 3;
  if (src_frame_stride < need || dst_frame_stride < frame) return (int)hipErrorInvalidValue;
  const long mx = src_frame_stride > dst_frame_stride ? src_frame_stride : dst_frame_stride;
  if (mx >= (1L << 31) || (long)n * mx >= (1L << 31)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  if (src == nullptr || dst == nullptr) return (int)hipErrorInvalidValue;
  const Geo g{static_cast<const uint8_t*>(src), static_cast<uint8_t*>(dst), (int)src_frame_stride,
              (int)dst_frame_stride, step, H, W, n};
  switch (code) {
    case 0: return launch<Perm<3, false>>(g, stream);
    case 1: return launch<Perm<3, true>>(g, stream);
    case 2: return launch<Perm<4, false>>(g, stream);
    case 3: return launch<Perm<4, true>>(g, stream);
    case 4: return launch<Mono<1, false>>(g, stream);
    case 5: return is_bigendian ? launch<Mono<2, true>>(g, stream) : launch<Mono<2, false>>(g, stream);
    case 6: return launch<Yuv<false>>(g, stream);
    case 7: return launch<Yuv<true>>(g, stream);
    case 8: return launch<Bayer<0, 0>>(g, stream);   // rggb
    case 9: return launch<Bayer<1, 1>>(g, stream);   // bggr
    case 10: return launch<Bayer<1, 0>>(g, stream);  // gbrg
    default: return launch<Bayer<0, 1>>(g, stream);  // grbg
  }
}
