// K28: rectify camera frames through a fixed-point map, byte for byte what
// ops/rectify.py rectify_numpy returns (that function is the specification; docs/precision.md
// "Rectification").  map[H][W] = (qx, qy) int32: the source position of an output pixel in 1/32
// pixel; the output is the 5-bit-weight bilinear blend of its four taps, a tap outside the
// frame counting as 0.
//
// A gather kernel.  One thread makes four consecutive output pixels of the packed frame (12
// output bytes: three dword stores where the frame's bytes are dword-aligned there, else twelve
// byte stores; the last one to three pixels of a frame whose H * W is no multiple of four are a
// per-pixel tail).  It reads its four map entries once (two 16-B loads), turns them into clamped
// tap offsets and weights, and then loops over a chunk of the batch's frames: the map costs 8 B
// per pixel, a frame 3 B in and 3 B out, so a map entry read per frame would more than double
// the traffic.  blockIdx.y strides over the chunks.
//
// The map is not trusted: tap coordinates are clamped into the frame (and the weight of a tap
// that was outside is zero), so no entry can make a load leave `src`.  A tap is three bytes at an
// arbitrary address; it is fetched with one dword load of the bytes [o, o + 4) -- or of
// [o - 1, o + 3) for the frame's last pixel, where the former would end one byte past the
// frame -- which needs a frame of at least 4 bytes; a 1 x 1 frame takes byte loads.  Neighbouring
// output pixels read neighbouring source pixels, so the gathers hit in L1/L2 and nothing is
// staged in LDS.
#include "tca_common.h"

namespace {

constexpr int kPx = 4;  // pixels per thread
constexpr int kThreads = 256;
constexpr int kMaxSide = 4096;
constexpr int kFrac = 5, kOne = 1 << kFrac;

constexpr int kChunk = 8;  // frames a thread makes from one read of its map entries

struct Px {
  int o00, o01, o10, o11;  // clamped tap offsets (bytes)
  int w00, w01, w10, w11;  // weights, zero for a tap outside the frame; they sum to <= 1024
};

__device__ __forceinline__ Px make_px(int qx, int qy, int H, int W) {
  const int ix = qx >> kFrac, iy = qy >> kFrac;  // arithmetic shifts
  const int ax = qx & (kOne - 1), ay = qy & (kOne - 1);
  const int x0 = min(max(ix, 0), W - 1), x1 = min(max(ix + 1, 0), W - 1);
  const int y0 = min(max(iy, 0), H - 1), y1 = min(max(iy + 1, 0), H - 1);
  const int wx0 = (ix >= 0 && ix < W) ? kOne - ax : 0, wx1 = (ix >= -1 && ix < W - 1) ? ax : 0;
  const int wy0 = (iy >= 0 && iy < H) ? kOne - ay : 0, wy1 = (iy >= -1 && iy < H - 1) ? ay : 0;
  Px p;
  p.o00 = (y0 * W + x0) * 3, p.o01 = (y0 * W + x1) * 3;
  p.o10 = (y1 * W + x0) * 3, p.o11 = (y1 * W + x1) * 3;
  p.w00 = wx0 * wy0, p.w01 = wx1 * wy0, p.w10 = wx0 * wy1, p.w11 = wx1 * wy1;
  return p;
}

// the three bytes of the pixel at byte offset o of frame s, as the low 24 bits
template <bool WIDE> __device__ __forceinline__ uint32_t load_px(const uint8_t* s, int o, int frame_bytes) {
  if constexpr (WIDE) {
    const int back = (o + 4 > frame_bytes) ? 1 : 0;  // only the frame's last pixel
    uint32_t v;
    __builtin_memcpy(&v, s + o - back, 4);
    return v >> (8 * back);
  } else {
    return (uint32_t)s[o] | (uint32_t)s[o + 1] << 8 | (uint32_t)s[o + 2] << 16;
  }
}

template <bool WIDE> __device__ __forceinline__ void blend(const uint8_t* s, const Px& p, int frame_bytes,
                                                           int (&o)[3]) {
  const uint32_t a = load_px<WIDE>(s, p.o00, frame_bytes), b = load_px<WIDE>(s, p.o01, frame_bytes);
  const uint32_t c = load_px<WIDE>(s, p.o10, frame_bytes), d = load_px<WIDE>(s, p.o11, frame_bytes);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int sh = 8 * ch;
    o[ch] = (p.w00 * (int)((a >> sh) & 0xffu) + p.w01 * (int)((b >> sh) & 0xffu) +
             p.w10 * (int)((c >> sh) & 0xffu) + p.w11 * (int)((d >> sh) & 0xffu) + (1 << (2 * kFrac - 1))) >>
            (2 * kFrac);
  }
}

// idx: a quad of the packed frame (adjacent lanes: adjacent quads).  32-bit offsets inside a
// frame (at most 4096 * 4096 * 3 bytes); the frame's base is a 64-bit product.
template <bool WIDE>
__global__ void __launch_bounds__(kThreads) rectify_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                           const int2* __restrict__ map, int H, int W, int n,
                                                           int chunk, int quads, int byte_stores) {
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx >= quads) return;
  const int hw = H * W, frame_bytes = hw * 3;
  const int p0 = idx * kPx;
  const int f0 = blockIdx.y * chunk, f1 = min(n, f0 + chunk);
  if (p0 + kPx <= hw) {
    const int4 m0 = reinterpret_cast<const int4*>(map)[2 * idx];  // (the launcher checked the alignment)
    const int4 m1 = reinterpret_cast<const int4*>(map)[2 * idx + 1];
    const Px px[kPx] = {make_px(m0.x, m0.y, H, W), make_px(m0.z, m0.w, H, W), make_px(m1.x, m1.y, H, W),
                        make_px(m1.z, m1.w, H, W)};
    for (int f = f0; f < f1; ++f) {
      const uint8_t* s = src + (size_t)f * frame_bytes;
      uint8_t* d = dst + (size_t)f * frame_bytes + (size_t)p0 * 3;
      int o[3 * kPx];
#pragma unroll
      for (int i = 0; i < kPx; ++i) {
        int c[3];
        blend<WIDE>(s, px[i], frame_bytes, c);
        o[3 * i] = c[0], o[3 * i + 1] = c[1], o[3 * i + 2] = c[2];
      }
      if ((reinterpret_cast<uintptr_t>(d) & 3) == 0 && !byte_stores) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
          reinterpret_cast<uint32_t*>(d)[i] = (uint32_t)o[4 * i] | (uint32_t)o[4 * i + 1] << 8 |
                                              (uint32_t)o[4 * i + 2] << 16 | (uint32_t)o[4 * i + 3] << 24;
      } else {
#pragma unroll
        for (int i = 0; i < 3 * kPx; ++i) d[i] = (uint8_t)o[i];
      }
    }
  } else {  // the frame's last one to three pixels
    for (int p = p0; p < hw; ++p) {
      const int2 m = map[p];
      const Px px = make_px(m.x, m.y, H, W);
      for (int f = f0; f < f1; ++f) {
        int c[3];
        blend<WIDE>(src + (size_t)f * frame_bytes, px, frame_bytes, c);
        uint8_t* d = dst + (size_t)f * frame_bytes + (size_t)p * 3;
        d[0] = (uint8_t)c[0], d[1] = (uint8_t)c[1], d[2] = (uint8_t)c[2];
      }
    }
  }
}

// The argument checks and the launch; chunk: frames per read of a thread's map entries.
int launch(const void* src, void* dst, const void* map, int H, int W, int n, int chunk, int byte_stores,
           hipStream_t stream) {
  if (H < 1 || H > kMaxSide || W < 1 || W > kMaxSide || n < 0 || chunk < 1) return (int)hipErrorInvalidValue;
  if (src == nullptr || dst == nullptr || map == nullptr || src == dst) return (int)hipErrorInvalidValue;
  if (reinterpret_cast<uintptr_t>(map) & 15) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const int quads = (H * W + kPx - 1) / kPx;
  const int groups = (n + chunk - 1) / chunk;
  const dim3 grid((quads + kThreads - 1) / kThreads, groups < 65535 ? groups : 65535);
  const int per = groups <= 65535 ? chunk : (n + 65534) / 65535;  // (n beyond 65535 chunks: longer chunks)
  const auto* s = static_cast<const uint8_t*>(src);
  auto* d = static_cast<uint8_t*>(dst);
  const auto* m = static_cast<const int2*>(map);
  if (H * W * 3 >= 4)
    rectify_kernel<true><<<grid, kThreads, 0, stream>>>(s, d, m, H, W, n, per, quads, byte_stores);
  else
    rectify_kernel<false><<<grid, kThreads, 0, stream>>>(s, d, m, H, W, n, per, quads, byte_stores);
  TCA_LAUNCH_CHECK();
}

}  // namespace

// dst[f] <- src[f] rectified through map, f < n.  src, dst: packed [n, H, W, 3] uint8 frames at
// any byte address, not the same buffer (they must not overlap); map: [H, W] (qx, qy) int32
// pairs, 16-byte aligned.  Nonzero (and no launch) for H or W outside 1..4096, n < 0, a null
// pointer, src == dst or a map that is not 16-byte aligned.  n == 0 launches nothing.  The file
// keeps no state.
TCA_API int tca_rectify(const void* src, void* dst, const void* map, int H, int W, int n, hipStream_t stream) {
  return launch(src, dst, map, H, W, n, kChunk, 0, stream);
}

// For measurements and tests (tools/rectify_bench.py, profiles/rectify): the same launch with the
// frames per read of a map entry (chunk >= 1) and the store path (byte_stores != 0: never the
// dword stores) given by the caller.  The same checks, the same bytes.
TCA_API int tca_rectify_variant(const void* src, void* dst, const void* map, int H, int W, int n, int chunk,
                                int byte_stores, hipStream_t stream) {
  return launch(src, dst, map, H, W, n, chunk, byte_stores ? 1 : 0, stream);
}
