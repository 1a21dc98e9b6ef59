// Baseline JPEG encoding on the GPU: rgb8 frames -> one JFIF file per frame.
// The definition, in integer arithmetic, is triton_client_amd/ops/jpeg_encode.py
// (encode_numpy); every kernel here reproduces it exactly.  The decoder's layouts are
// reused: the int32[16] geometry record of csrc/runtime/jpeg_entropy.cpp, the
// component-planar block order and natural-order int16 coefficients of jpeg.hip.
//
// Kernel 1 (jpeg_fdct_kernel<HS,VS>): one workgroup per MCU, one thread per pixel.
//   libjpeg's fixed-point RGB -> YCbCr on edge-clamped coordinates, chroma box
//   downsampling through LDS, then jfdctint's row and column passes (one thread per
//   row / column of each of the MCU's blocks) and libjpeg's quantisation.
// Kernel 2 / 4 (jpeg_enc_kernel<WRITE>): one lane per restart interval walks its MCUs'
//   blocks (a block's 64 coefficients are one 128-B line, staged in a per-lane LDS row)
//   and Huffman-codes them.  WRITE = false counts the interval's bytes (stuffing,
//   padding and its RST marker included); WRITE = true runs the same code again and
//   stores them at the interval's offset, so no worst-case scratch is needed.
// Kernel 3 (jpeg_enc_scan_kernel): one workgroup per frame: exclusive scan of the
//   interval sizes, the frame's length (or -needed when it exceeds the caller's cap),
//   the header copied from a small device buffer, and EOI.
//
// The Huffman and zigzag tables, the quantisation tables and the header come from
// device buffers the caller filled once; this file keeps no state.
#include "tca_common.h"

namespace {

struct EncGeom {
  int W, H, HS, VS, mcux, mcuy;
  int nblocks;       // blocks per frame (all components)
  int bw0;           // luma block grid width
  int boff1, boff2;  // first Cb / Cr block within a frame
};

// geom: W, H, nc, hmax, vmax, mcux, mcuy, h0, v0, h1, v1, h2, v2, nblocks.  Three
// components, luma at (hmax, vmax), chroma at (1, 1): 4:4:4, 4:2:2 or 4:2:0.
bool make_enc_geom(const int32_t* s, EncGeom& g) {
  g.W = s[0];
  g.H = s[1];
  g.HS = s[3];
  g.VS = s[4];
  g.mcux = s[5];
  g.mcuy = s[6];
  if (s[2] != 3 || g.W <= 0 || g.H <= 0 || g.W > 65535 || g.H > 65535) return false;
  if (s[7] != g.HS || s[8] != g.VS || s[9] != 1 || s[10] != 1 || s[11] != 1 || s[12] != 1) return false;
  if (!((g.HS == 1 && g.VS == 1) || (g.HS == 2 && g.VS == 1) || (g.HS == 2 && g.VS == 2))) return false;
  if (g.mcux != (g.W + 8 * g.HS - 1) / (8 * g.HS) || g.mcuy != (g.H + 8 * g.VS - 1) / (8 * g.VS)) return false;
  const long long nm = (long long)g.mcux * g.mcuy;
  const long long nb = nm * (g.HS * g.VS + 2);
  if (nb != s[13] || nb * 64 * 8 > 0x7fffffffLL) return false;  // byte counts stay in int32
  g.nblocks = (int)nb;
  g.bw0 = g.mcux * g.HS;
  g.boff1 = (int)(nm * g.HS * g.VS);
  g.boff2 = g.boff1 + (int)nm;
  return true;
}

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// One 1-D pass of libjpeg's jfdctint over d[0], d[stride], ... d[7*stride], in place.
template <bool FIRST>
__device__ __forceinline__ void fdct8(int* d, int stride) {
  const int d0 = d[0], d1 = d[stride], d2 = d[2 * stride], d3 = d[3 * stride];
  const int d4 = d[4 * stride], d5 = d[5 * stride], d6 = d[6 * stride], d7 = d[7 * stride];
  const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6;
  const int t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  constexpr int SH = FIRST ? 11 : 15;  // CONST_BITS -/+ PASS1_BITS
  if (FIRST) {
    d[0] = (t10 + t11) << 2;
    d[4 * stride] = (t10 - t11) << 2;
  } else {
    d[0] = descale(t10 + t11, 2);
    d[4 * stride] = descale(t10 - t11, 2);
  }
  int z1 = (t12 + t13) * 4433;
  d[2 * stride] = descale(z1 + t13 * 6270, SH);
  d[6 * stride] = descale(z1 - t12 * 15137, SH);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7 * stride] = descale(a4 + z1 + z3, SH);
  d[5 * stride] = descale(a5 + z2 + z4, SH);
  d[3 * stride] = descale(a6 + z2 + z3, SH);
  d[stride] = descale(a7 + z1 + z4, SH);
}

// frames uint8 [n][frame_stride] (rows of W*3), qt int32 [2][64] natural order,
// coef int16 [n][coef_stride_blocks][64].  blockDim = 64*HS*VS, grid = n*mcux*mcuy.
template <int HS, int VS>
__global__ __launch_bounds__(64 * HS * VS) void jpeg_fdct_kernel(const uint8_t* __restrict__ frames,
                                                                  const int* __restrict__ qt,
                                                                  int16_t* __restrict__ coef, EncGeom g,
                                                                  long long frame_stride,
                                                                  long long coef_stride_blocks) {
  constexpr int NY = HS * VS, NB = NY + 2, PW = 8 * HS, PH = 8 * VS, NT = 64 * HS * VS;
  __shared__ int blk[NB][64];
  __shared__ int cfull[2][PH][PW];  // full-resolution Cb, Cr of the MCU (subsampled layouts)
  const int t = threadIdx.x;
  const int per = g.mcux * g.mcuy;
  const int f = blockIdx.x / per;
  const int m = blockIdx.x - f * per;
  const int my = m / g.mcux, mx = m - my * g.mcux;
  {
    const int px = t % PW, py = t / PW;
    const int gx = min(mx * PW + px, g.W - 1), gy = min(my * PH + py, g.H - 1);
    const uint8_t* p = frames + (long long)f * frame_stride + ((long long)gy * g.W + gx) * 3;
    const int r = p[0], gg = p[1], b = p[2];
    const int y = (19595 * r + 38470 * gg + 7471 * b + 32768) >> 16;
    const int cb = (-11059 * r - 21709 * gg + 32768 * b + (128 << 16) + 32767) >> 16;
    const int cr = (32768 * r - 27439 * gg - 5329 * b + (128 << 16) + 32767) >> 16;
    const int k = (py & 7) * 8 + (px & 7);
    blk[(py >> 3) * HS + (px >> 3)][k] = y - 128;
    if constexpr (NY == 1) {
      blk[1][k] = cb - 128;
      blk[2][k] = cr - 128;
    } else {
      cfull[0][py][px] = cb;
      cfull[1][py][px] = cr;
    }
  }
  __syncthreads();
  if constexpr (NY > 1) {
    if (t < 128) {  // libjpeg's box filters; the bias alternates along the output row
      const int c = t >> 6, oy = (t >> 3) & 7, ox = t & 7;
      int v;
      if constexpr (VS == 2) {
        v = (cfull[c][2 * oy][2 * ox] + cfull[c][2 * oy][2 * ox + 1] + cfull[c][2 * oy + 1][2 * ox] +
             cfull[c][2 * oy + 1][2 * ox + 1] + 1 + (ox & 1)) >> 2;
      } else {
        v = (cfull[c][oy][2 * ox] + cfull[c][oy][2 * ox + 1] + (ox & 1)) >> 1;
      }
      blk[NY + c][oy * 8 + ox] = v - 128;
    }
    __syncthreads();
  }
  if (t < NB * 8) fdct8<true>(&blk[t >> 3][(t & 7) * 8], 1);  // rows
  __syncthreads();
  if (t < NB * 8) fdct8<false>(&blk[t >> 3][t & 7], 8);  // columns
  __syncthreads();
  for (int i = t; i < NB * 64; i += NT) {
    const int b = i >> 6, k = i & 63;
    const int q8 = qt[(b < NY ? 0 : 64) + k] << 3;
    const int v = blk[b][k];
    const int mag = (abs(v) + (q8 >> 1)) / q8;
    int bi;
    if (b < NY) {
      bi = (my * VS + b / HS) * g.bw0 + mx * HS + b % HS;
    } else {
      bi = (b == NY ? g.boff1 : g.boff2) + my * g.mcux + mx;
    }
    coef[((long long)f * coef_stride_blocks + bi) * 64 + k] = (int16_t)(v < 0 ? -mag : mag);
  }
}

// offsets into the table buffer (ops/jpeg_encode.py device_tables): code << 5 | length
constexpr int kTabDc0 = 0, kTabDc1 = 12, kTabAc0 = 24, kTabAc1 = 280, kTabZigzag = 536, kTabSize = 600;

// Bit accumulator of one restart interval.  WRITE = false only counts.
template <bool WRITE>
struct BitSink {
  uint64_t acc = 0;
  int nb = 0;      // pending bits in acc (< 8 between calls)
  int count = 0;   // bytes produced
  uint8_t* p = nullptr;
  int room = 0;    // bytes this interval may store
  __device__ __forceinline__ void byte(unsigned v) {
    if constexpr (WRITE) {
      if (count < room) p[count] = (uint8_t)v;
    }
    ++count;
  }
  __device__ __forceinline__ void put(unsigned code, int len) {  // len <= 27
    acc = (acc << len) | code;
    nb += len;
    while (nb >= 8) {
      const unsigned v = (unsigned)(acc >> (nb - 8)) & 0xffu;
      byte(v);
      if (v == 0xffu) byte(0);
      nb -= 8;
    }
  }
  __device__ __forceinline__ void flush() {  // pad the last byte with 1-bits
    if (nb) {
      const int pad = 8 - nb;
      put((1u << pad) - 1u, pad);
    }
  }
};

__device__ __forceinline__ int bit_length(int v) { return v ? 32 - __clz(v) : 0; }

// coef int16 [n][coef_stride_blocks][64]; seg_size / seg_off int32 [n][nseg];
// out uint8 [n][cap]; lens int32 [n] (from the scan kernel; < 0: the frame is skipped).
// blockDim = 64, grid = n * segblocks with segblocks = ceil(nseg / 64).
template <bool WRITE>
__global__ __launch_bounds__(64) void jpeg_enc_kernel(const int16_t* __restrict__ coef,
                                                       const int* __restrict__ tabs, EncGeom g,
                                                       long long coef_stride_blocks, int restart,
                                                       int* __restrict__ seg_size, const int* __restrict__ seg_off,
                                                       int nseg, int segblocks, int hlen, uint8_t* __restrict__ out,
                                                       long long cap, const int* __restrict__ lens) {
  __shared__ int tab[kTabSize];
  __shared__ uint32_t line[64][33];  // one block per lane, rows padded to 33 dwords
  const int lane = threadIdx.x;
  for (int i = lane; i < kTabSize; i += 64) tab[i] = tabs[i];
  __syncthreads();
  const int f = blockIdx.x / segblocks;
  const int s = (blockIdx.x - f * segblocks) * 64 + lane;
  if (s >= nseg) return;
  BitSink<WRITE> sink;
  if constexpr (WRITE) {
    const int len = lens[f];
    if (len < 0) return;  // the frame does not fit: nothing of it is written
    const int off = hlen + seg_off[(long long)f * nseg + s];
    sink.p = out + (long long)f * cap + off;
    sink.room = len - 2 - off;  // up to the frame's EOI
  }
  const int NY = g.HS * g.VS, NB = NY + 2;
  const int nm = g.mcux * g.mcuy;
  const int m0 = s * restart, m1 = min(m0 + restart, nm);
  const int16_t* fc = coef + (long long)f * coef_stride_blocks * 64;
  const uint32_t* mine = line[lane];
  auto at = [&](int i) { return (int)(int16_t)(mine[i >> 1] >> ((i & 1) * 16)); };  // coefficient i of the staged block
  int pred0 = 0, pred1 = 0, pred2 = 0;
  for (int m = m0; m < m1; ++m) {
    const int my = m / g.mcux, mx = m - my * g.mcux;
    for (int b = 0; b < NB; ++b) {
      int bi;
      if (b < NY) {
        bi = (my * g.VS + b / g.HS) * g.bw0 + mx * g.HS + b % g.HS;
      } else {
        bi = (b == NY ? g.boff1 : g.boff2) + m;
      }
      const uint4* src = (const uint4*)(fc + (long long)bi * 64);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const uint4 v = src[i];
        line[lane][4 * i] = v.x;
        line[lane][4 * i + 1] = v.y;
        line[lane][4 * i + 2] = v.z;
        line[lane][4 * i + 3] = v.w;
      }
      const int dcb = b < NY ? kTabDc0 : kTabDc1, acb = b < NY ? kTabAc0 : kTabAc1;
      const int dc = at(0);
      int d;
      if (b < NY) {
        d = dc - pred0;
        pred0 = dc;
      } else if (b == NY) {
        d = dc - pred1;
        pred1 = dc;
      } else {
        d = dc - pred2;
        pred2 = dc;
      }
      {
        const int n = min(bit_length(abs(d)), 11);  // the DC tables end at category 11 (tca_jpeg_fdct stays below)
        const unsigned bits = (unsigned)(d < 0 ? d - 1 : d) & ((1u << n) - 1u);
        const int e = tab[dcb + n];
        sink.put(((unsigned)(e >> 5) << n) | bits, (e & 31) + n);
      }
      int run = 0;
      for (int k = 1; k < 64; ++k) {
        const int v = at(tab[kTabZigzag + k] & 63);
        if (v == 0) {
          ++run;
          continue;
        }
        while (run > 15) {
          const int e = tab[acb + 0xf0];
          sink.put((unsigned)(e >> 5), e & 31);
          run -= 16;
        }
        const int n = min(bit_length(abs(v)), 10);  // the AC tables end at category 10
        const unsigned bits = (unsigned)(v < 0 ? v - 1 : v) & ((1u << n) - 1u);
        const int e = tab[acb + (run << 4 | n)];
        sink.put(((unsigned)(e >> 5) << n) | bits, (e & 31) + n);
        run = 0;
      }
      if (run) {
        const int e = tab[acb];
        sink.put((unsigned)(e >> 5), e & 31);
      }
    }
  }
  sink.flush();
  if (s != nseg - 1) {  // RSTm, not stuffed
    sink.byte(0xff);
    sink.byte(0xd0 + (s & 7));
  }
  if constexpr (!WRITE) seg_size[(long long)f * nseg + s] = sink.count;
}

// blockDim = 256, grid = n.
__global__ __launch_bounds__(256) void jpeg_enc_scan_kernel(const int* __restrict__ seg_size,
                                                             int* __restrict__ seg_off, int nseg,
                                                             const uint8_t* __restrict__ hdr, int hlen,
                                                             uint8_t* __restrict__ out, long long cap,
                                                             int* __restrict__ lens) {
  __shared__ int lds[256 / 64 + 1];
  const int f = blockIdx.x;
  int base = 0;
  for (int s0 = 0; s0 < nseg; s0 += 256) {
    const int s = s0 + threadIdx.x;
    const int v = s < nseg ? seg_size[(long long)f * nseg + s] : 0;
    int total;
    const int ex = tca::block_excl_scan(v, lds, &total);
    if (s < nseg) seg_off[(long long)f * nseg + s] = base + ex;
    base += total;
  }
  const long long need = (long long)hlen + base + 2;
  uint8_t* o = out + (long long)f * cap;
  if (need <= cap) {
    for (int i = threadIdx.x; i < hlen; i += 256) o[i] = hdr[i];
    if (threadIdx.x == 0) {
      o[need - 2] = 0xff;
      o[need - 1] = 0xd9;
      lens[f] = (int)need;
    }
  } else if (threadIdx.x == 0) {
    lens[f] = (int)-need;
  }
}

bool enc_args(const int16_t* coef, const int32_t* geom, EncGeom& g, long long coef_stride_blocks, int restart, int nseg, int n) {
  if (!make_enc_geom(geom, g) || n <= 0 || restart <= 0 || coef_stride_blocks < g.nblocks) return false;
  if ((uintptr_t)coef & 15) return false;  // blocks are read as 16-B vectors
  const long long nm = (long long)g.mcux * g.mcuy;
  if (nseg != (nm + restart - 1) / restart) return false;
  return (long long)n * ((nseg + 63) / 64) <= 0x7fffffffLL;
}

}  // namespace

// n rgb8 frames -> quantised coefficients.  frames uint8 [n][frame_stride] (packed rows
// of W*3 bytes), qt int32 [2][64] (luma, chroma; natural order, 1..255),
// coef int16 [n][coef_stride_blocks][64].
TCA_API int tca_jpeg_fdct(const uint8_t* frames, const int* qt, int16_t* coef, const int32_t* geom,
                          long long frame_stride, long long coef_stride_blocks, int n, hipStream_t stream) {
  EncGeom g;
  if (!make_enc_geom(geom, g) || n <= 0) return (int)hipErrorInvalidValue;
  if (frame_stride < (long long)g.W * g.H * 3 || coef_stride_blocks < g.nblocks) return (int)hipErrorInvalidValue;
  const long long grid = (long long)n * g.mcux * g.mcuy;
  if (grid > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  if (g.HS == 1) {
    jpeg_fdct_kernel<1, 1><<<(unsigned)grid, 64, 0, stream>>>(frames, qt, coef, g, frame_stride, coef_stride_blocks);
  } else if (g.VS == 1) {
    jpeg_fdct_kernel<2, 1><<<(unsigned)grid, 128, 0, stream>>>(frames, qt, coef, g, frame_stride, coef_stride_blocks);
  } else {
    jpeg_fdct_kernel<2, 2><<<(unsigned)grid, 256, 0, stream>>>(frames, qt, coef, g, frame_stride, coef_stride_blocks);
  }
  TCA_LAUNCH_CHECK();
}

// Bytes of every restart interval (restart MCUs each; nseg per frame) of n frames into
// seg_size int32 [n][nseg].  tabs: int32 [600], the code tables and the zigzag order.
TCA_API int tca_jpeg_enc_size(const int16_t* coef, const int* tabs, const int32_t* geom, long long coef_stride_blocks,
                              int restart, int* seg_size, int nseg, int n, hipStream_t stream) {
  EncGeom g;
  if (!enc_args(coef, geom, g, coef_stride_blocks, restart, nseg, n)) return (int)hipErrorInvalidValue;
  const int segblocks = (nseg + 63) / 64;
  jpeg_enc_kernel<false><<<(unsigned)(n * segblocks), 64, 0, stream>>>(coef, tabs, g, coef_stride_blocks, restart,
                                                                       seg_size, nullptr, nseg, segblocks, 0, nullptr,
                                                                       0, nullptr);
  TCA_LAUNCH_CHECK();
}

// seg_size -> seg_off (exclusive scan per frame), lens[b] = the file's bytes or
// -needed when that exceeds cap; a frame that fits gets its header (hdr, hlen bytes) and EOI.
TCA_API int tca_jpeg_enc_scan(const int* seg_size, int* seg_off, int nseg, const uint8_t* hdr, int hlen, uint8_t* out,
                              long long cap, int* lens, int n, hipStream_t stream) {
  if (n <= 0 || nseg <= 0 || hlen <= 0 || cap <= 0 || cap > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  jpeg_enc_scan_kernel<<<(unsigned)n, 256, 0, stream>>>(seg_size, seg_off, nseg, hdr, hlen, out, cap, lens);
  TCA_LAUNCH_CHECK();
}

// Every interval of every frame that fits, written at out[b] + hlen + seg_off[b][s].
TCA_API int tca_jpeg_enc_write(const int16_t* coef, const int* tabs, const int32_t* geom, long long coef_stride_blocks,
                               int restart, const int* seg_off, int nseg, int hlen, uint8_t* out, long long cap,
                               const int* lens, int n, hipStream_t stream) {
  EncGeom g;
  if (!enc_args(coef, geom, g, coef_stride_blocks, restart, nseg, n) || hlen <= 0 || cap <= 0 || cap > 0x7fffffffLL) {
    return (int)hipErrorInvalidValue;
  }
  const int segblocks = (nseg + 63) / 64;
  jpeg_enc_kernel<true><<<(unsigned)(n * segblocks), 64, 0, stream>>>(coef, tabs, g, coef_stride_blocks, restart,
                                                                      nullptr, seg_off, nseg, segblocks, hlen, out, cap,
                                                                      lens);
  TCA_LAUNCH_CHECK();
}
