// K27 — the cloud as a camera-frame depth image: project every point into the image and keep,
// per pixel, the nearest depth of the points whose splat square covers it.
//
// Batched over B <= 64 clouds that share one field layout.  Raw PointCloud2 bytes are read in
// place (tca_cloud_load.h: 16-byte record, dwords or bytes, chosen from the alignment of the
// base pointer and of each frame's offset).  M = float32(P @ T) [3, 4] is the only calibration
// the device sees.
//
//   reset    the key plane uint32[B][H][W] is set to 0xFFFFFFFF, 16 bytes per lane.
//   points   one lane per point, blocks of 256, blockIdx.y = frame.  A valid point does an
//            atomicMin of its key (the depth in output units, or the bits of the positive float
//            depth) into every pixel of its (2 splat + 1)^2 square, clipped to the image.
//   convert  four pixels per lane: the plane becomes the output image, uint16 (one 8-byte store)
//            or float from the key bits (one 16-byte store); an untouched pixel becomes 0 or the
//            quiet NaN 0x7FC00000.  The images of a batch lie back to back, so only the last
//            lane of the launch has a tail.
//
// The reset belongs to the launch: a relaunch or a graph replay gives the same bytes.  Only
// integer atomics are used, so no output depends on the order blocks run in.  The arithmetic is
// the float32 definition of ops/depth_image.py, every operation rounded on its own: contraction
// to FMA is switched off for this file, the division is IEEE.
#include "tca_cloud_load.h"
#include "tca_common.h"

#include <cmath>

#pragma clang fp contract(off)

using namespace tca;

namespace {

constexpr int kBlock = 256;
constexpr int kMaxFrames = 64;
constexpr int kMaxSide = 4096;
constexpr int kMaxSplat = 4;
constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr uint32_t kNanBits = 0x7FC00000u;
constexpr int kEnc16U = 0, kEnc32F = 1;

struct DepthArgs {
  int step;
  int off[4];  // x, y, z, -1
  int fast;    // tca_cloud_load.h
  float m[12];
  int W, H;
  int enc;
  float scale, min_depth;
  int splat;
};

__global__ void __launch_bounds__(kBlock) depth_reset_kernel(uint32_t* __restrict__ plane, long n) {
  const long i = ((long)blockIdx.x * kBlock + threadIdx.x) * 4;
  if (i + 4 <= n) {
    *reinterpret_cast<uint4*>(plane + i) = make_uint4(kEmpty, kEmpty, kEmpty, kEmpty);
  } else {
    for (long j = i; j < n; ++j) plane[j] = kEmpty;
  }
}

__global__ void __launch_bounds__(kBlock) depth_points_kernel(
    const uint8_t* __restrict__ data, long data_bytes, const long* __restrict__ frame_off,
    const int* __restrict__ frame_n, DepthArgs a, uint32_t* __restrict__ plane) {
  const int b = blockIdx.y;
  const int n = frame_n[b];
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  const long foff = frame_off[b];
  const long at = foff + i * a.step;
  // a record outside the buffer is not read
  if (!(i < n && foff >= 0 && foff <= data_bytes && at + a.step <= data_bytes)) return;

  uint32_t raw[4] = {0u, 0u, 0u, 0u};
  cloud_load_fields(data + at, a.off, cloud_frame_path(a.fast, foff), raw);
  const float x = __uint_as_float(raw[0]), y = __uint_as_float(raw[1]), z = __uint_as_float(raw[2]);

  const float w = ((a.m[8] * x + a.m[9] * y) + a.m[10] * z) + a.m[11];
  const float pa = ((a.m[0] * x + a.m[1] * y) + a.m[2] * z) + a.m[3];
  const float pb = ((a.m[4] * x + a.m[5] * y) + a.m[6] * z) + a.m[7];
  const float u = pa / w, v = pb / w;
  // a NaN compares false
  if (!(w >= a.min_depth && u >= 0.f && u < (float)a.W && v >= 0.f && v < (float)a.H)) return;
  const int px = (int)u, py = (int)v;  // truncation: floor of a value in [0, W)

  uint32_t key;
  if (a.enc == kEnc16U) {
    float t = w * a.scale;
    t = t < 65536.f ? t : 65536.f;
    const int d = (int)rintf(t);  // v_rndne_f32: half to even
    if (d < 1 || d > 65535) return;  // beyond the range: dropped, never clamped
    key = (uint32_t)d;
  } else {
    key = __float_as_uint(w);  // w >= min_depth > 0: positive floats order as their bits
  }

  const int x0 = max(px - a.splat, 0), x1 = min(px + a.splat, a.W - 1);
  const int y0 = max(py - a.splat, 0), y1 = min(py + a.splat, a.H - 1);
  uint32_t* frame = plane + (long)b * a.H * a.W;
  for (int yy = y0; yy <= y1; ++yy) {
    uint32_t* row = frame + (long)yy * a.W;
    for (int xx = x0; xx <= x1; ++xx) atomicMin(row + xx, key);
  }
}

// n pixels of the whole batch; out16: uint16[n], out32: uint32[n] (float bits)
__global__ void __launch_bounds__(kBlock) depth_convert_kernel(const uint32_t* __restrict__ plane, long n, int enc,
                                                               void* __restrict__ out) {
  const long i = ((long)blockIdx.x * kBlock + threadIdx.x) * 4;
  if (i >= n) return;
  if (i + 4 <= n) {
    uint4 k = *reinterpret_cast<const uint4*>(plane + i);
    if (enc == kEnc16U) {
      const uint32_t p0 = k.x == kEmpty ? 0u : k.x, p1 = k.y == kEmpty ? 0u : k.y;
      const uint32_t p2 = k.z == kEmpty ? 0u : k.z, p3 = k.w == kEmpty ? 0u : k.w;
      *reinterpret_cast<uint2*>((uint16_t*)out + i) = make_uint2(p0 | (p1 << 16), p2 | (p3 << 16));
    } else {
      k.x = k.x == kEmpty ? kNanBits : k.x;
      k.y = k.y == kEmpty ? kNanBits : k.y;
      k.z = k.z == kEmpty ? kNanBits : k.z;
      k.w = k.w == kEmpty ? kNanBits : k.w;
      *reinterpret_cast<uint4*>((uint32_t*)out + i) = k;
    }
    return;
  }
  for (long j = i; j < n; ++j) {  // the last lane's tail: fewer than four pixels
    const uint32_t k = plane[j];
    if (enc == kEnc16U) ((uint16_t*)out)[j] = (uint16_t)(k == kEmpty ? 0u : k);
    else ((uint32_t*)out)[j] = k == kEmpty ? kNanBits : k;
  }
}

}  // namespace

// data: device bytes, data_bytes of them (no record outside is read); frame_off long[B] (bytes) / frame_n int[B]:
// device; max_n: the largest frame_n (host, sizes the grid); offsets of x, y, z in a record of FLOAT32 fields.
// m float[12] (row-major [3, 4]): HOST, copied into the launch.  encoding: 0 = 16UC1, 1 = 32FC1.  plane:
// B * H * W uint32 of workspace, 16-B aligned, reset here on the stream.  out: B * H * W pixels of 2 or 4 bytes,
// the images back to back, 16-B aligned.
TCA_API int tca_depth_image(const void* data, long data_bytes, const long* frame_off, const int* frame_n, int batch,
                            int max_n, int point_step, int off_x, int off_y, int off_z, const float* m, int width,
                            int height, int encoding, float scale, float min_depth, int splat, void* plane, void* out,
                            hipStream_t stream) {
  if (batch < 1 || batch > kMaxFrames || max_n < 0 || point_step <= 0 || data_bytes < 0 ||
      data_bytes >= 0x80000000L)
    return (int)hipErrorInvalidValue;
  if (width < 1 || width > kMaxSide || height < 1 || height > kMaxSide || splat < 0 || splat > kMaxSplat ||
      (encoding != kEnc16U && encoding != kEnc32F))
    return (int)hipErrorInvalidValue;
  if (!std::isfinite(scale) || !(scale > 0.f) || !std::isfinite(min_depth) || !(min_depth > 0.f))
    return (int)hipErrorInvalidValue;
  if (m == nullptr || frame_off == nullptr || frame_n == nullptr || plane == nullptr || out == nullptr ||
      (max_n > 0 && data == nullptr))
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)plane & 15) != 0 || ((uintptr_t)out & 15) != 0 || ((uintptr_t)frame_off & 7) != 0 ||
      ((uintptr_t)frame_n & 3) != 0)
    return (int)hipErrorInvalidValue;
  DepthArgs a;
  a.step = point_step;
  a.off[0] = off_x; a.off[1] = off_y; a.off[2] = off_z; a.off[3] = -1;
  a.fast = cloud_fast_path(data, point_step, a.off, true);
  if (a.fast < 0) return (int)hipErrorInvalidValue;
  for (int j = 0; j < 12; ++j) a.m[j] = m[j];
  a.W = width;
  a.H = height;
  a.enc = encoding;
  a.scale = scale;
  a.min_depth = min_depth;
  a.splat = splat;
  const long n_px = (long)batch * height * width;  // <= 2^30
  const unsigned px_blocks = (unsigned)((n_px + 4L * kBlock - 1) / (4L * kBlock));
  depth_reset_kernel<<<px_blocks, kBlock, 0, stream>>>((uint32_t*)plane, n_px);
  if (int e = (int)hipGetLastError()) return e;
  if (max_n > 0) {
    const dim3 grid((max_n + kBlock - 1) / kBlock, batch);
    depth_points_kernel<<<grid, kBlock, 0, stream>>>((const uint8_t*)data, data_bytes, frame_off, frame_n, a,
                                                     (uint32_t*)plane);
    if (int e = (int)hipGetLastError()) return e;
  }
  depth_convert_kernel<<<px_blocks, kBlock, 0, stream>>>((const uint32_t*)plane, n_px, encoding, out);
  TCA_LAUNCH_CHECK();
}
