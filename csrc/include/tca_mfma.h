// Shared primitives of the MFMA kernels (gfx950 / CDNA4 only).
//
// The GPU tests compare tiles of different kernel families bit for bit, and the
// models rely on "same bits whichever kernel takes the layer".  That holds only
// while every family rounds, orders its products and activates the same way, so
// hx3, wino, s2sp, the BEV necks, spconv and the pillar encoders take these
// helpers from this one place.  conv_mfma.hip, c3_fused.hip, image.hip and
// yolo_detect.hip still carry private copies, which must keep the same expressions.
#pragma once
#include "tca_common.h"

namespace tca {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));   // one lane's A / B fragment of mfma_f32_16x16x32_bf16
typedef float f32x4 __attribute__((ext_vector_type(4)));     // one lane's 16x16 accumulator
typedef float f32x16 __attribute__((ext_vector_type(16)));   // one lane's 32x32 accumulator

// Epilogue activation: 0 none, 1 relu, 2 silu, 3 leaky(0.1).  Every family uses
// these expressions (a kernel and its twin in another family must give the same
// bits); conv_mfma.hip's own act_fn is this one plus mish (4).
__device__ __forceinline__ float act_fn(float v, int act) {
  switch (act) {
    case 1: return fmaxf(v, 0.f);
    case 2: return v / (1.f + __expf(-v));
    case 3: return v > 0.f ? v : 0.1f * v;
    default: return v;
  }
}

// ---- fp32 mode: split products.  x = hi + lo with hi = bf16_rne(x),
// lo = bf16_rne(x - hi): |x - hi - lo| <= 2^-17 |x|.
__device__ __forceinline__ void split_bf16(float v, __bf16& hi, __bf16& lo) {
  hi = (__bf16)v;
  lo = (__bf16)(v - (float)hi);
}

__device__ __forceinline__ void split8(const float4& x0, const float4& x1, bf16x8& hi, bf16x8& lo) {
  const float v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const __bf16 h = (__bf16)v[e];
    hi[e] = h;
    lo[e] = (__bf16)(v[e] - (float)h);
  }
}

// x * w ~= xl*wh + xh*wl + xh*wh (the dropped xl*wl is <= 2^-16 |x w|): three
// mfma_f32_16x16x32_bf16 into one fp32 accumulator, in THIS order: lo*hi, hi*lo,
// hi*hi.  fp32 addition does not associate, so the order is part of every fp32-mode
// kernel's result; kernels that issue the products themselves (product-major over
// several accumulators) keep the same order per accumulator.
__device__ __forceinline__ void mfma3(f32x4& acc, const bf16x8& bh, const bf16x8& bl, const bf16x8& ah,
                                      const bf16x8& al) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bl, ah, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, al, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, ah, acc, 0, 0, 0);
}

// Pair storage (PairTag in tca_common.h): 8 channels as {hi bf16 x 8 | lo bf16 x 8}
// = 32 B, the same bytes and element offsets as 8 fp32 values.  pair_split8 writes
// what a consumer's MFMA reads as stored (no VALU split on the read), so its
// rounding is split8's; pair_join8 reads 8 channels at p back as hi + lo.
__device__ __forceinline__ void pair_split8(const float* v, uint4& hi, uint4& lo) {
  __bf16 h[8], l[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    h[e] = (__bf16)v[e];
    l[e] = (__bf16)(v[e] - (float)h[e]);
  }
  hi = *reinterpret_cast<const uint4*>(h);
  lo = *reinterpret_cast<const uint4*>(l);
}

__device__ __forceinline__ void pair_join8(const float* p, float* v) {
  const uint4 hq = *reinterpret_cast<const uint4*>(p);
  const uint4 lq = *reinterpret_cast<const uint4*>(p + 4);
  const __bf16* h = reinterpret_cast<const __bf16*>(&hq);
  const __bf16* l = reinterpret_cast<const __bf16*>(&lq);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (float)h[e] + (float)l[e];
}

// ---- global -> LDS DMA, 16 B per lane: the wave's 64 pieces land contiguously
// at the wave-uniform LDS address l (lane i at l + 16 * i).  Three forms:
//  * glds16: the builtin.  hipcc counts it, and where a ds_read might alias a DMA
//    in flight it inserts a conservative vmcnt(0) of its own.  Used by the bf16
//    kernels (the glds tiles, the halo kernel, the bf16 neck).
//  * glds16_asm (tca_common.h): the same instruction from inline asm, which hipcc
//    neither counts nor guards: the caller waits with its own counted wait_vm<N>()
//    and a barrier before reading the destination.  Used by the x3 glds rings, whose
//    fragment reads sit between DMAs of younger stages that must stay in flight, and
//    for the fp32 neck's head bias.
//  * bdma16: buffer_load ... lds through a buffer descriptor, also uncounted:
//    per-lane 32-bit voffset plus a scalar soffset, and an offset at or past the
//    descriptor's num_records reads zeros, so padding taps and M / N tails cost
//    no select and no memory traffic (the xb, hx, hx3, wino and fp32 neck kernels).
typedef __attribute__((address_space(3))) void* lds_void_t;
typedef __attribute__((address_space(1))) void* gbl_void_t;

__device__ __forceinline__ void glds16(const void* g, unsigned char* l) {
  __builtin_amdgcn_global_load_lds((gbl_void_t)g, (lds_void_t)l, 16, 0, 0);
}

__device__ __forceinline__ void bdma16(unsigned voff, __amdgpu_buffer_rsrc_t rsrc, const void* l, unsigned soff) {
  const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)l);
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %4 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(voff), "s"(rsrc), "s"(dst), "s"(soff)
               : "memory");
}

// Buffer offset that reads zeros (bdma16, raw buffer loads): every launcher that
// builds a descriptor rejects tensors of 2 GiB or more, so num_records < 2^31 <=
// kOutOfRange and the descriptor's range check fails for it.
constexpr unsigned kOutOfRange = 0x80000000u;

// s_waitcnt vmcnt(N): at most this wave's N youngest vector-memory ops (the DMAs
// above included) still in flight.  gfx9 encoding: vmcnt[3:0] in bits 3:0 and
// vmcnt[5:4] in bits 15:14; 0x0F70 leaves expcnt (6:4) and lgkmcnt (11:8) at
// "no wait".  The field has 6 bits.
template <int N>
__device__ __forceinline__ void wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | 0x0F70);
}

// ---- LDS slot swizzles (conflict-free ds_read_b128 fragment reads)
// [rows][64 B] tile (BK = 32 bf16): byte offset of 16-B chunk c (0..3) of row r
__device__ __forceinline__ int swz(int r, int c) { return r * 64 + ((c ^ ((r >> 2) & 3)) << 4); }
// [rows][128 B] tile of bf16 (BK = 64), one 16-B slot per lane group: slot ^= swz2(row)
__device__ __forceinline__ int swz2(int row) { return (row >> 1) & 7; }
// [rows][128 B] tile of 32 fp32 / 4 pair chunks, a lane group reading slots 2fq and
// 2fq + 1 (the x3 glds tiles): slot ^= swz3(row), rows at any 16-row fragment base
__device__ __forceinline__ int swz3(int row) { return (row ^ (row >> 3)) & 7; }
// the same layout with the swizzle 16-row periodic (swz3 of the row within its
// fragment), so fragment i of a wave is a constant offset from one per-lane base
// (the xb tiles and the fp32 neck)
__device__ __forceinline__ int swzp(int row) { return swz3(row & 15); }
// halo tiles (hx, hx3): slot swizzle of halo column hx (0..17), 3 bits per column
// pair, conflict-free at the three tap shifts kx = 0..2 (found by exhaustive search)
__device__ __forceinline__ int hswz(int hx) { return (0xb29108 >> (3 * (hx >> 1))) & 7; }

}  // namespace tca
