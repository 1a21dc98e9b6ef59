// K38 — the holes of K27's depth image filled: IP-Basic's chain of morphological filters and a median (Ku, Harakeh,
// Waslander 2018) on the uint32 key plane tca_depth_image leaves in its workspace.  ops/depth_image.py (fill_numpy)
// has the definition; every stage selects a key and never computes one, so the bytes are equal, not near.  E =
// 0xFFFFFFFF is the empty pixel and the largest key: a dilation of the paper's inverted depth is a minimum of keys.
//
//   1  A = min of K over the diamond |dx| + |dy| <= k
//   2  B = min of A over the square k, C = max of B over the square k             (closing)
//   3  D = C where C != E, else min of C over the square h                        (h = 0: skipped)
//   4  F = D where D != E, else min of D over the square g                        (g = 0: skipped)
//   5  G = E where F == E, else the median of F's (2m+1)^2 window, or F where that is E   (m = 0: skipped)
//
// A tap outside the image is skipped in 1..4 and clamped in 5.
//
// Batched over the B planes of a launch, blockIdx.z = plane.  A workgroup of 256 lanes owns a tile of 64 x 32 pixels
// and stages the keys of the tile plus a halo in LDS: two buffers of (64 + 2 halo) x (32 + 2 halo) dwords with an odd
// pitch, ping-ponged between barriers; every stage shrinks the part that is valid by its radius.
//
//   front    stages 1..3, halo 3k + h (<= 19: 56 KiB); alone it writes the tile's D keys to the scratch plane
//   back     stages 4..5, halo g + m (<= 17: 51 KiB); writes the finished image, uint16 or float bits
//   fused    both in one launch, halo 3k + h + g + m (<= 36: 111 KiB of gfx950's 160: one workgroup per CU)
//
//   load     the region row by row, E outside the image.  A wave that saw a key raises an LDS flag: with no key in
//            the region every stage gives E, the tile is written empty and nothing else runs (skip_empty = 1).
//   diamond  one lane per pixel, 2k + 1 row segments of widths 1, 3, .. 2k + 1, .. 1.
//   squares  separable, a row pass then a column pass.  A lane owns four consecutive outputs along the filter's
//            direction and walks their 2r + 4 taps once: (2r + 4) / 4 LDS reads per output, not 2r + 1.  The lanes of
//            a wave lie across the direction: consecutive columns in a column pass, consecutive rows in a row pass,
//            where the odd pitch keeps them on different banks.
//   edges    a position outside the image holds what the next stage's operator ignores: every column pass (and the
//            diamond) writes E there before a minimum and 0 before the maximum, so a skipped tap neither dilates nor
//            erodes.  The row passes write what they find: a column pass reads its own column only.
//   fills    stages 3 and 4 run their column pass in place: a lane reads its pixel's own key and keeps it unless it is E.
//   median   one lane per tile pixel: the window from LDS with clamped coordinates, the network of tca_median.h.
//
// Plain C++, integer compares, vector stores, no atomics: nothing depends on the order workgroups run in, and a
// relaunch or a graph replay gives the same bytes.  No position outside a plane is read or written.
#include "tca_common.h"
#include "tca_median.h"

using namespace tca;

namespace {

constexpr int kBlock = 256;
constexpr int kTileW = 64, kTileH = 32;
constexpr int kMaxFrames = 64;  // the limits of tca_depth_image (depth_image.hip)
constexpr int kMaxSide = 4096;
constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr uint32_t kNanBits = 0x7FC00000u;
constexpr int kEnc16U = 0, kEnc32F = 1;
constexpr int kMaxK = 4, kMaxHole = 7, kMaxLarge = 15, kMaxMedian = 2;
constexpr int kFront = 1, kBack = 2;  // FillArgs::stages

struct FillArgs {
  int W, H, enc;
  int k, h, g, m;
  int stages;  // kFront | kBack
  int skip;    // skip_empty
};

struct Tile {
  int gx0, gy0;  // the image position of the region's first dword
  int W, H;
  int pitch;
  __device__ __forceinline__ bool inside(int lx, int ly) const {
    const int gx = gx0 + lx, gy = gy0 + ly;
    return gx >= 0 && gx < W && gy >= 0 && gy < H;
  }
};

// dst(a, s) = fin(a, s, op of src(a, s - r .. s + r)) for a in [a0, a1), s in [s0, s1); (a, s) lies at a * sa + s * ss.
// src must be valid for s in [s0 - r, s1 + r).  dst may be what fin reads at (a, s), never src.
template <bool kMax, typename Fin>
__device__ __forceinline__ void line_pass(const uint32_t* src, uint32_t* dst, int a0, int a1, int s0, int s1, int r,
                                          int sa, int ss, Fin fin) {
  const int na = a1 - a0, n = na * ((s1 - s0 + 3) >> 2);
  const uint32_t neutral = kMax ? 0u : kEmpty;
  for (int it = threadIdx.x; it < n; it += kBlock) {
    const int gi = it / na, a = a0 + (it - gi * na), s = s0 + 4 * gi;
    const int cnt = min(4, s1 - s);   // the outputs of this group
    const int last = 2 * r + cnt - 1;  // its last tap: none past s1 + r
    const uint32_t* p = src + a * sa + (s - r) * ss;
    uint32_t o0 = neutral, o1 = neutral, o2 = neutral, o3 = neutral;
    for (int j = 0; j <= last; ++j) {  // (j and r are the same for every lane: these are scalar branches)
      const uint32_t v = p[j * ss];
      if (j <= 2 * r) o0 = kMax ? max(o0, v) : min(o0, v);
      if (j >= 1 && j <= 2 * r + 1) o1 = kMax ? max(o1, v) : min(o1, v);
      if (j >= 2 && j <= 2 * r + 2) o2 = kMax ? max(o2, v) : min(o2, v);
      if (j >= 3) o3 = kMax ? max(o3, v) : min(o3, v);
    }
    uint32_t* q = dst + a * sa + s * ss;
    q[0] = fin(a, s, o0);
    if (cnt > 1) q[ss] = fin(a, s + 1, o1);
    if (cnt > 2) q[2 * ss] = fin(a, s + 2, o2);
    if (cnt > 3) q[3 * ss] = fin(a, s + 3, o3);
  }
}

// One square of half-width r on the part of `cur` that is valid from margin mg inwards (RW x RH dwords): a row pass
// into oth, then a column pass back into cur.  kKeep = true: only the E keys of cur are replaced.  A position outside
// the image gets `outside`.  mg grows by r.
template <bool kMax, bool kKeep>
__device__ __forceinline__ void square_pass(uint32_t* cur, uint32_t* oth, const Tile& t, int RW, int RH, int& mg,
                                            int r, uint32_t outside) {
  const int pitch = t.pitch;
  line_pass<kMax>(cur, oth, mg, RH - mg, mg + r, RW - mg - r, r, pitch, 1, [](int, int, uint32_t v) { return v; });
  __syncthreads();
  if (kKeep) {
    const uint32_t* own = cur;
    line_pass<kMax>(oth, cur, mg + r, RW - mg - r, mg + r, RH - mg - r, r, 1, pitch, [&](int x, int y, uint32_t v) {
      const uint32_t c = own[y * pitch + x];
      return !t.inside(x, y) ? outside : (c != kEmpty ? c : v);
    });
  } else {
    line_pass<kMax>(oth, cur, mg + r, RW - mg - r, mg + r, RH - mg - r, r, 1, pitch,
                    [&](int x, int y, uint32_t v) { return t.inside(x, y) ? v : outside; });
  }
  __syncthreads();
  mg += r;
}

template <int kM>
__device__ __forceinline__ uint32_t window_median(const uint32_t* f, const Tile& t, int gx, int gy) {
  constexpr int kSide = 2 * kM + 1;
  uint32_t p[kSide * kSide];
#pragma unroll
  for (int dy = -kM; dy <= kM; ++dy) {
    const int ly = min(max(gy + dy, 0), t.H - 1) - t.gy0;
#pragma unroll
    for (int dx = -kM; dx <= kM; ++dx) {
      const int lx = min(max(gx + dx, 0), t.W - 1) - t.gx0;
      p[(dy + kM) * kSide + dx + kM] = f[ly * t.pitch + lx];
    }
  }
  if constexpr (kM == 1) return median9(p);
  else return median25(p);
}

__global__ void __launch_bounds__(kBlock) depth_fill_kernel(const uint32_t* __restrict__ keys, FillArgs a,
                                                            uint32_t* __restrict__ keys_out, void* __restrict__ out) {
  extern __shared__ uint32_t lds[];
  __shared__ int flag;
  const bool front = (a.stages & kFront) != 0, back = (a.stages & kBack) != 0;
  const int halo = (front ? 3 * a.k + a.h : 0) + (back ? a.g + a.m : 0);
  const int RW = kTileW + 2 * halo, RH = kTileH + 2 * halo;
  const int tid = threadIdx.x;
  Tile t;
  t.W = a.W; t.H = a.H;
  t.pitch = RW | 1;
  t.gx0 = blockIdx.x * kTileW - halo;
  t.gy0 = blockIdx.y * kTileH - halo;
  const int pitch = t.pitch;
  uint32_t* cur = lds;
  uint32_t* oth = lds + pitch * RH;
  const long frame = (long)blockIdx.z * a.H * a.W;
  const uint32_t* plane = keys + frame;

  if (tid == 0) flag = 0;
  __syncthreads();

  // ------------------------------------------------------------------------------------ load
  bool seen = false;
  for (int i = tid; i < RW * RH; i += kBlock) {
    const int ly = i / RW, lx = i - ly * RW;
    uint32_t v = kEmpty;
    if (t.inside(lx, ly)) v = plane[(long)(t.gy0 + ly) * a.W + t.gx0 + lx];
    seen |= v != kEmpty;
    cur[ly * pitch + lx] = v;
  }
  if (seen) flag = 1;  // (every writer stores the same value)
  __syncthreads();
  const bool empty = a.skip && flag == 0;  // the same for the whole workgroup

  int mg = 0;
  if (!empty && front) {
    // --------------------------------------------------------------------------------- diamond
    const int k = a.k, nw = RW - 2 * k, nh = RH - 2 * k;
    for (int i = tid; i < nw * nh; i += kBlock) {
      const int r = i / nw, lx = k + (i - r * nw), ly = k + r;
      uint32_t v = kEmpty;
      for (int dy = -k; dy <= k; ++dy) {
        const int w = k - abs(dy);
        const uint32_t* row = cur + (ly + dy) * pitch + lx;
        for (int dx = -w; dx <= w; ++dx) v = min(v, row[dx]);
      }
      oth[ly * pitch + lx] = t.inside(lx, ly) ? v : kEmpty;
    }
    __syncthreads();
    { uint32_t* s = cur; cur = oth; oth = s; }
    mg = k;
    // --------------------------------------------------------------------------------- closing, small holes
    square_pass<false, false>(cur, oth, t, RW, RH, mg, k, 0u);  // (what the maximum ignores)
    square_pass<true, false>(cur, oth, t, RW, RH, mg, k, kEmpty);
    if (a.h > 0) square_pass<false, true>(cur, oth, t, RW, RH, mg, a.h, kEmpty);
  }
  // --------------------------------------------------------------------------------- large holes
  if (!empty && back && a.g > 0) square_pass<false, true>(cur, oth, t, RW, RH, mg, a.g, kEmpty);

  // ------------------------------------------------------------------------ median and the tile's pixels
  for (int i = tid; i < kTileW * kTileH; i += kBlock) {
    const int y = i / kTileW, x = i - y * kTileW;
    const int gx = blockIdx.x * kTileW + x, gy = blockIdx.y * kTileH + y;
    if (gx >= a.W || gy >= a.H) continue;
    uint32_t v = kEmpty;
    if (!empty) {
      v = cur[(halo + y) * pitch + halo + x];
      if (back && v != kEmpty && a.m > 0) {
        const uint32_t med = a.m == 1 ? window_median<1>(cur, t, gx, gy) : window_median<2>(cur, t, gx, gy);
        if (med != kEmpty) v = med;
      }
    }
    const long at = frame + (long)gy * a.W + gx;
    if (!back) keys_out[at] = v;
    else if (a.enc == kEnc16U) ((uint16_t*)out)[at] = (uint16_t)(v == kEmpty ? 0u : v);
    else ((uint32_t*)out)[at] = v == kEmpty ? kNanBits : v;
  }
}

size_t fill_lds_bytes(int halo) {
  const int RW = kTileW + 2 * halo, RH = kTileH + 2 * halo;
  return (size_t)2 * (RW | 1) * RH * sizeof(uint32_t);
}

}  // namespace

// keys: the planes tca_depth_image left in its workspace, uint32[B][H][W], keys_bytes of them.  encoding: 0 = 16UC1,
// 1 = 32FC1.  k (1..4), hole (0..7), large (0..15), median (0..2): the radii of ops/depth_image.py's fill_numpy.
// fused: 0, stages 1..3 into `scratch` (another B * H * W uint32, scratch_bytes of it) and stages 4..5 from there, two
// launches; 1, one launch and no scratch (it may be null).  With large = median = 0 there is one launch either way.
// skip_empty: 1, a tile with no key within its halo is written empty at once (0: measurements; the same bytes).
// out: B * H * W pixels of 2 or 4 bytes, the images back to back, out_bytes of it; nothing past them is written.
// Every buffer is 4-byte aligned and none overlaps another.  What does not fit is refused before any launch.
TCA_API int tca_depth_fill(const void* keys, long keys_bytes, int batch, int width, int height, int encoding, int k,
                           int hole, int large, int median, int fused, int skip_empty, void* scratch,
                           long scratch_bytes, void* out, long out_bytes, hipStream_t stream) {
  if (batch < 1 || batch > kMaxFrames || width < 1 || width > kMaxSide || height < 1 || height > kMaxSide ||
      (encoding != kEnc16U && encoding != kEnc32F))
    return (int)hipErrorInvalidValue;
  if (k < 1 || k > kMaxK || hole < 0 || hole > kMaxHole || large < 0 || large > kMaxLarge || median < 0 ||
      median > kMaxMedian || (fused != 0 && fused != 1) || (skip_empty != 0 && skip_empty != 1))
    return (int)hipErrorInvalidValue;
  const long n_px = (long)batch * height * width;  // <= 2^30
  const bool one = fused == 1 || (large == 0 && median == 0);
  if (keys == nullptr || out == nullptr || keys_bytes < 4 * n_px || out_bytes < n_px * (encoding == kEnc16U ? 2 : 4))
    return (int)hipErrorInvalidValue;
  if (!one && (scratch == nullptr || scratch_bytes < 4 * n_px || scratch == keys || scratch == out))
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)keys & 3) != 0 || ((uintptr_t)out & 3) != 0 || ((uintptr_t)scratch & 3) != 0 || keys == out)
    return (int)hipErrorInvalidValue;
  FillArgs a;
  a.W = width; a.H = height; a.enc = encoding;
  a.k = k; a.h = hole; a.g = large; a.m = median;
  a.skip = skip_empty;
  const dim3 grid((width + kTileW - 1) / kTileW, (height + kTileH - 1) / kTileH, batch);
  const int front_halo = 3 * k + hole, back_halo = large + median;
  if (one) {
    const size_t lds = fill_lds_bytes(front_halo + back_halo);
    if (lds > 64 * 1024) {  // above the default limit of dynamic LDS: ask for it (a host call, nothing on the stream)
      if (int e = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(depth_fill_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
        return e;
    }
    a.stages = kFront | kBack;
    depth_fill_kernel<<<grid, kBlock, lds, stream>>>((const uint32_t*)keys, a, nullptr, out);
    TCA_LAUNCH_CHECK();
  }
  a.stages = kFront;
  depth_fill_kernel<<<grid, kBlock, fill_lds_bytes(front_halo), stream>>>((const uint32_t*)keys, a, (uint32_t*)scratch,
                                                                         nullptr);
  if (int e = (int)hipGetLastError()) return e;
  a.stages = kBack;
  depth_fill_kernel<<<grid, kBlock, fill_lds_bytes(back_halo), stream>>>((const uint32_t*)scratch, a, nullptr, out);
  TCA_LAUNCH_CHECK();
}
