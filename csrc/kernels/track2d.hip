// K25 — tracking camera detections from one frame to the next: ByteTrack's association
// (Zhang et al., ECCV 2022) made deterministic, bit for bit the float32 definition of
// ops/track2d.py (every operation rounded on its own: contraction to FMA is switched off
// for this file; the divisions are IEEE, the build has no fast-math).  Detections choose in
// descending score order (the host orders the rows); a high-score row may match any live
// track, a low-score row only one matched in the previous frame, and only rows with the
// birth flag start a track.  The cost is the IoU of the row with the predicted box; a
// fixed-gain constant-velocity filter with a smoothed size stands in for the Kalman filter.
//
// One launch walks F frames in order against the persistent state.  A tracker is serial
// over frames and, inside a frame, over detections, so ONE workgroup does the work:
// blockDim = the capacity rounded up to a wave, lane t owns slot t.  The state (13 arrays
// of capacity words) is loaded into LDS once, lives there for the whole launch and is
// stored once.
//
// Per frame: the frame's rows are staged in LDS (the row's gate, min_iou or min_iou_low by
// its "high" flag, goes into its pad word then, and its area over the score, which the
// kernel never reads: the host compared it); every lane predicts its slot and keeps the
// predicted box's corners and area in registers; then, one row at a time, every lane
// evaluates its slot's IoU and the workgroup takes the maximum of the key
// (IoU bits << 32 | ~slot) — an IoU is non-negative, so its bit pattern orders as an
// integer, and the inverted slot breaks ties towards the lower slot; no key is 0, which
// stands for "no candidate": a wave max by shuffles, one LDS word per wave (double-buffered
// by the step's parity: one barrier per row), and every lane reduces the <= 8 wave maxima
// itself.  The owner of the winning slot claims it and updates it after the loop.  Births
// rank the free slots and the unmatched rows with the birth flag with ballot prefix counts
// (lowest free slot to the first such row) and write the new slots through LDS.
//
// Static LDS at the caps (512 slots, 512 rows): 13 * 2,048 (state) + 16,384 (rows) + 1,024
// (match) + 1,024 (free list) + 128 (wave maxima) + 32 (ballot counts) = 45,216 B of the
// 65,536 B a workgroup may have; 1,024 slots would need 69,632 B for state and rows alone.
#include "tca_common.h"

#pragma clang fp contract(off)

using namespace tca;

namespace {

constexpr int kMaxCap = 512;     // slots
constexpr int kMaxDets = 512;    // rows per frame
constexpr int kMaxFrames = 64;   // frames per launch
constexpr int kHeader = 4;       // state words in front of the arrays: next_id, overflow, 2 pad
constexpr int kFields = 13;      // id, label, cx, cy, w, h, vx, vy, px, py, pt, age, hits
constexpr int kValid = 1, kHigh = 2, kBirth = 4;
constexpr unsigned long long kNone = 0ull;

struct TrackOffsets { int off[kMaxFrames + 1]; };

// area: (x2-x1)*(y2-y1), over the row's score; gate: over its pad word.  Both filled in LDS.
struct DetRow { float x1, y1, x2, y2, area; int label, flags; float gate; };

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}

// Exclusive rank of the lanes with `flag` over the workgroup and their number, from ballots.
// cnt: blockDim/64 ints of LDS; two barriers, the first also orders the caller's earlier LDS writes.
__device__ __forceinline__ int block_rank(bool flag, int* cnt, int* total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const unsigned long long m = __ballot(flag);
  __syncthreads();  // the previous use of cnt is over
  if (lane == 0) cnt[wid] = __popcll(m);
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < nw; ++w) {
    const int c = cnt[w];
    before += w < wid ? c : 0;
    all += c;
  }
  *total = all;
  return before + __popcll(m & ((1ull << lane) - 1ull));
}

__global__ void __launch_bounds__(kMaxCap) track2d_kernel(
    const uint4* __restrict__ rows, TrackOffsets offs, int n_frames, const float* __restrict__ dts,
    const uint8_t* __restrict__ resets, int* __restrict__ state, int cap, int max_age, float min_iou,
    float min_iou_low, float alpha, float beta, int4* __restrict__ out) {
  __shared__ int s_id[kMaxCap], s_label[kMaxCap], s_age[kMaxCap], s_hits[kMaxCap];
  __shared__ float s_cx[kMaxCap], s_cy[kMaxCap], s_w[kMaxCap], s_h[kMaxCap], s_vx[kMaxCap], s_vy[kMaxCap],
      s_px[kMaxCap], s_py[kMaxCap], s_pt[kMaxCap];
  __shared__ __attribute__((aligned(16))) DetRow s_det[kMaxDets];
  __shared__ short s_match[kMaxDets];     // the slot a row matched, -1
  __shared__ short s_free[kMaxCap];       // the free slots in ascending order
  __shared__ unsigned long long s_red[2][kMaxCap / 64];
  __shared__ int s_cnt[kMaxCap / 64];

  const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wid = t >> 6, nw = nt >> 6;
  const bool own = t < cap;
  int* const sw[kFields] = {s_id, s_label, (int*)s_cx, (int*)s_cy, (int*)s_w, (int*)s_h, (int*)s_vx, (int*)s_vy,
                            (int*)s_px, (int*)s_py, (int*)s_pt, s_age, s_hits};
  if (own) {
#pragma unroll
    for (int k = 0; k < kFields; ++k) sw[k][t] = state[kHeader + k * cap + t];
  }
  int next_id = state[0], overflow = state[1];  // every lane keeps the same copy

  for (int f = 0; f < n_frames; ++f) {
    const int n0 = offs.off[f], n = offs.off[f + 1] - n0;
    const float dt = dts[f];
    const bool reset = resets[f] != 0;
    __syncthreads();  // the previous frame is done with s_det, s_match, and its births are written
    for (int i = t; i < n; i += nt) {
      const uint4 a = rows[2 * (long)(n0 + i)], b = rows[2 * (long)(n0 + i) + 1];
      DetRow d;
      d.x1 = __uint_as_float(a.x); d.y1 = __uint_as_float(a.y); d.x2 = __uint_as_float(a.z); d.y2 = __uint_as_float(a.w);
      d.area = (d.x2 - d.x1) * (d.y2 - d.y1);
      d.label = (int)b.y; d.flags = (int)b.z;
      d.gate = (d.flags & kHigh) ? min_iou : min_iou_low;
      s_det[i] = d;
      s_match[i] = -1;
    }
    // 1, 2: reset, predict (the lane's own slot); the predicted box stays in registers
    int id = 0, label = 0;
    bool fresh = false;  // matched (or born) in the previous frame: a low row may keep it
    float tx1 = 0.f, tx2 = 0.f, ty1 = 0.f, ty2 = 0.f, t_area = 0.f;
    if (own) {
      id = reset ? 0 : s_id[t];
      label = s_label[t];
      if (id != 0) {
        const float cx = s_cx[t] + s_vx[t] * dt, cy = s_cy[t] + s_vy[t] * dt;
        const float w = s_w[t], h = s_h[t];
        s_cx[t] = cx;
        s_cy[t] = cy;
        s_pt[t] = s_pt[t] + dt;
        tx1 = cx - 0.5f * w; tx2 = cx + 0.5f * w;
        ty1 = cy - 0.5f * h; ty2 = cy + 0.5f * h;
        t_area = (tx2 - tx1) * (ty2 - ty1);
        fresh = s_age[t] == 0;
      }
    }
    const bool live = id != 0;
    __syncthreads();  // s_det is staged

    // 3: match, one row at a time
    int mine = -1;  // the row that claimed this lane's slot
    int step = 0;
    for (int i = 0; i < n; ++i) {
      const DetRow d = s_det[i];  // the same address in every lane: an LDS broadcast
      if (!(d.flags & kValid)) continue;  // uniform
      unsigned long long key = kNone;
      if (live && mine < 0 && label == d.label && (fresh || (d.flags & kHigh))) {
        float iw = (d.x2 < tx2 ? d.x2 : tx2) - (d.x1 > tx1 ? d.x1 : tx1);
        float ih = (d.y2 < ty2 ? d.y2 : ty2) - (d.y1 > ty1 ? d.y1 : ty1);
        iw = iw > 0.f ? iw : 0.f;
        ih = ih > 0.f ? ih : 0.f;
        const float inter = iw * ih;
        const float u = (d.area + t_area) - inter;
        const float q = u > 0.f ? inter / u : 0.f;
        if (q >= d.gate) key = ((unsigned long long)__float_as_uint(q) << 32) | (unsigned)~t;  // closed gate; NaN: no
      }
      key = wave_max_u64(key);
      unsigned long long* red = s_red[step & 1];
      ++step;
      if (lane == 0) red[wid] = key;
      __syncthreads();
      unsigned long long best = red[0];
      for (int w = 1; w < nw; ++w) {
        const unsigned long long v = red[w];
        best = v > best ? v : best;
      }
      if (best != kNone && (int)~(unsigned)best == t) {
        mine = i;
        s_match[i] = (short)t;
      }
    }

    // 4, 5: update the matched slot, age the others
    bool is_free = own && !live;
    if (live) {
      if (mine >= 0) {
        const DetRow d = s_det[mine];
        const float dcx = (d.x1 + d.x2) * 0.5f, dcy = (d.y1 + d.y2) * 0.5f;
        float vx = s_vx[t], vy = s_vy[t];
        const float pt = s_pt[t], w = s_w[t], h = s_h[t];
        const int hits = s_hits[t];
        if (pt > 0.f) {
          const float vmx = (dcx - s_px[t]) / pt, vmy = (dcy - s_py[t]) / pt;
          if (hits == 1) {
            vx = vmx;
            vy = vmy;
          } else {
            vx = vx + alpha * (vmx - vx);
            vy = vy + alpha * (vmy - vy);
          }
        }
        s_vx[t] = vx; s_vy[t] = vy;
        s_cx[t] = dcx; s_cy[t] = dcy; s_px[t] = dcx; s_py[t] = dcy;
        s_w[t] = w + beta * ((d.x2 - d.x1) - w);
        s_h[t] = h + beta * ((d.y2 - d.y1) - h);
        s_pt[t] = 0.f;
        s_age[t] = 0;
        s_hits[t] = hits + 1;
        out[n0 + mine] = make_int4(id, hits + 1, (int)__float_as_uint(vx), (int)__float_as_uint(vy));
      } else {
        const int age = s_age[t] + 1;
        s_age[t] = age;
        if (age > max_age) {
          id = 0;
          is_free = true;
        }
      }
    }
    if (own) s_id[t] = id;

    // 6: births — the r-th unmatched row with the birth flag takes the r-th free slot
    int n_free;
    const int fr = block_rank(is_free, s_cnt, &n_free);  // (its first barrier: s_match, s_id are written)
    if (is_free) s_free[fr] = (short)t;
    int born = 0;  // unmatched rows with the birth flag so far
    for (int i0 = 0; i0 < n; i0 += nt) {
      const int i = i0 + t;
      bool want = false, unmatched = false;
      if (i < n) {
        const int fl = s_det[i].flags;
        unmatched = s_match[i] < 0;
        want = unmatched && (fl & kValid) && (fl & kBirth);
      }
      int n_want;
      const int r = born + block_rank(want, s_cnt, &n_want);  // (its barriers: s_free is written)
      born += n_want;
      if (want && r < n_free) {
        const DetRow d = s_det[i];
        const int s = s_free[r];
        const float dcx = (d.x1 + d.x2) * 0.5f, dcy = (d.y1 + d.y2) * 0.5f;
        s_id[s] = next_id + r;
        s_label[s] = d.label;
        s_cx[s] = dcx; s_cy[s] = dcy; s_px[s] = dcx; s_py[s] = dcy;
        s_w[s] = d.x2 - d.x1; s_h[s] = d.y2 - d.y1;
        s_vx[s] = 0.f; s_vy[s] = 0.f;
        s_pt[s] = 0.f;
        s_age[s] = 0;
        s_hits[s] = 1;
        out[n0 + i] = make_int4(next_id + r, 1, 0, 0);
      } else if (unmatched) {
        out[n0 + i] = make_int4(0, 0, 0, 0);  // invalid, no birth flag, or no free slot
      }
    }
    const int taken = born < n_free ? born : n_free;
    next_id += taken;
    overflow += born - taken;
  }

  __syncthreads();
  if (own) {
#pragma unroll
    for (int k = 0; k < kFields; ++k) state[kHeader + k * cap + t] = sw[k][t];
  }
  if (t == 0) {
    state[0] = next_id;
    state[1] = overflow;
  }
}

}  // namespace

// rows: device, 32 B per detection (x1, y1, x2, y2, score float; label, flags int; 1 pad word), 16-byte aligned,
// each frame's in descending score order.  det_off: HOST int[n_frames + 1], validated here and passed to the
// kernel by value.  dt float[n_frames], reset uint8[n_frames]: device.  state: device int[4 + 13 * capacity]
// (next_id, overflow, 2 pad; then id, label, cx, cy, w, h, vx, vy, px, py, pt, age, hits).  out: device int4 per
// detection (track id, hits, vx bits, vy bits).  Nothing is launched, and nothing written, on a bad argument.
TCA_API int tca_track2d(const void* rows, const int* det_off, int n_frames, const float* dt, const uint8_t* reset,
                        int* state, int capacity, int max_age, float min_iou, float min_iou_low, float alpha,
                        float beta, void* out, hipStream_t stream) {
  if (capacity < 1 || capacity > kMaxCap || n_frames < 0 || n_frames > kMaxFrames || max_age < 0)
    return (int)hipErrorInvalidValue;
  if (det_off == nullptr || state == nullptr || det_off[0] != 0) return (int)hipErrorInvalidValue;
  TrackOffsets offs;
  for (int f = 0; f <= kMaxFrames; ++f) offs.off[f] = 0;
  for (int f = 0; f < n_frames; ++f) {
    const long d = (long)det_off[f + 1] - (long)det_off[f];
    if (d < 0 || d > kMaxDets) return (int)hipErrorInvalidValue;
    offs.off[f + 1] = det_off[f + 1];
  }
  if (((uintptr_t)rows & 15) != 0 || ((uintptr_t)out & 15) != 0 || ((uintptr_t)state & 3) != 0 ||
      ((uintptr_t)dt & 3) != 0)
    return (int)hipErrorInvalidValue;
  if (n_frames == 0) return 0;
  if (dt == nullptr || reset == nullptr) return (int)hipErrorInvalidValue;
  if (offs.off[n_frames] > 0 && (rows == nullptr || out == nullptr)) return (int)hipErrorInvalidValue;
  const int threads = (capacity + kWave - 1) / kWave * kWave;
  track2d_kernel<<<1, threads, 0, stream>>>((const uint4*)rows, offs, n_frames, dt, reset, state, capacity, max_age,
                                            min_iou, min_iou_low, alpha, beta, (int4*)out);
  TCA_LAUNCH_CHECK();
}
