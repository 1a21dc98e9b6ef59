// K24 — tracking LiDAR detections from one cloud to the next: the CenterPoint paper's
// greedy closest-centre association on velocity-compensated positions, bit for bit the
// float32 definition of ops/track3d.py (every operation rounded on its own: contraction
// to FMA is switched off for this file; the one division is IEEE, the build has no
// fast-math).
//
// One launch walks F frames in order against the persistent state.  A tracker is serial
// over frames and, inside a frame, over detections (a detection does not give way to a
// later, closer one), so ONE workgroup does the work: blockDim = the capacity rounded up
// to a wave, lane t owns slot t.  The state (11 arrays of capacity words) is loaded into
// LDS once, lives there for the whole launch and is stored once.
//
// Per frame: the frame's rows are staged in LDS (the detection's squared gate is looked up
// then, into the row's first pad word); every lane predicts its slot; then, one detection
// at a time, every lane evaluates its slot's cost and the workgroup takes the minimum of
// the key (cost bits << 32 | slot) — costs are non-negative, so their bit patterns order
// as integers, and the low word breaks ties towards the lower slot: a wave min by
// shuffles, one LDS word per wave (double-buffered by the detection's parity: one barrier
// per detection), and every lane reduces the <= 16 wave minima itself.  The owner of the
// winning slot claims it and updates it after the loop.  Births rank the free slots and
// the unmatched detections with ballot prefix counts (lowest free slot to the first
// unmatched detection) and write the new slots through LDS.
#include "tca_common.h"

#pragma clang fp contract(off)

using namespace tca;

namespace {

constexpr int kMaxCap = 1024;    // slots
constexpr int kMaxDets = 512;    // detections per frame
constexpr int kMaxFrames = 64;   // frames per launch
constexpr int kHeader = 4;       // state words in front of the arrays: next_id, overflow, 2 pad
constexpr int kFields = 11;      // id, label, x, y, vx, vy, px, py, pt, age, hits
constexpr int kValid = 1, kHasVel = 2;
constexpr unsigned long long kNone = ~0ull;

struct TrackOffsets { int off[kMaxFrames + 1]; };

struct DetRow { float x, y, vx, vy; int label, flags; float gate; int pad; };  // gate: filled in LDS

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(v, o, 64);
    v = t < v ? t : v;
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

__global__ void __launch_bounds__(kMaxCap) track3d_kernel(
    const uint4* __restrict__ rows, TrackOffsets offs, int n_frames, const float* __restrict__ dts,
    const uint8_t* __restrict__ resets, const float* __restrict__ gates, int n_gates, int* __restrict__ state,
    int cap, int max_age, float alpha, int4* __restrict__ out) {
  __shared__ int s_id[kMaxCap], s_label[kMaxCap], s_age[kMaxCap], s_hits[kMaxCap];
  __shared__ float s_x[kMaxCap], s_y[kMaxCap], s_vx[kMaxCap], s_vy[kMaxCap], s_px[kMaxCap], s_py[kMaxCap],
      s_pt[kMaxCap];
  __shared__ __attribute__((aligned(16))) DetRow s_det[kMaxDets];
  __shared__ short s_match[kMaxDets];     // the slot a detection matched, -1
  __shared__ short s_free[kMaxCap];       // the free slots in ascending order
  __shared__ unsigned long long s_red[2][kMaxCap / 64];
  __shared__ int s_cnt[kMaxCap / 64];

  const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wid = t >> 6, nw = nt >> 6;
  const bool own = t < cap;
  int* const sw[kFields] = {s_id, s_label, (int*)s_x, (int*)s_y, (int*)s_vx, (int*)s_vy, (int*)s_px, (int*)s_py,
                            (int*)s_pt, s_age, s_hits};
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
      d.x = __uint_as_float(a.x); d.y = __uint_as_float(a.y); d.vx = __uint_as_float(a.z); d.vy = __uint_as_float(a.w);
      d.label = (int)b.x; d.flags = (int)b.y;
      d.gate = gates[(unsigned)d.label < (unsigned)(n_gates - 1) ? d.label : n_gates - 1];
      d.pad = 0;
      s_det[i] = d;
      s_match[i] = -1;
    }
    // 1, 2: reset, predict (the lane's own slot)
    int id = 0, label = 0;
    float x = 0.f, y = 0.f;
    if (own) {
      id = reset ? 0 : s_id[t];
      label = s_label[t];
      if (id != 0) {
        x = s_x[t] + s_vx[t] * dt;
        y = s_y[t] + s_vy[t] * dt;
        s_x[t] = x;
        s_y[t] = y;
        s_pt[t] = s_pt[t] + dt;
      }
    }
    const bool live = id != 0;
    __syncthreads();  // s_det is staged

    // 3: match, one detection at a time
    int mine = -1;  // the detection that claimed this lane's slot
    int step = 0;
    for (int i = 0; i < n; ++i) {
      const DetRow d = s_det[i];  // the same address in every lane: an LDS broadcast
      if (!(d.flags & kValid)) continue;  // uniform
      unsigned long long key = kNone;
      if (live && mine < 0 && label == d.label) {
        const float dx = d.x - x, dy = d.y - y;
        const float c = dx * dx + dy * dy;
        if (c <= d.gate) key = ((unsigned long long)__float_as_uint(c) << 32) | (unsigned)t;  // closed gate; NaN: no
      }
      key = wave_min_u64(key);
      unsigned long long* red = s_red[step & 1];
      ++step;
      if (lane == 0) red[wid] = key;
      __syncthreads();
      unsigned long long best = red[0];
      for (int w = 1; w < nw; ++w) {
        const unsigned long long v = red[w];
        best = v < best ? v : best;
      }
      if (best != kNone && (int)(unsigned)best == t) {
        mine = i;
        s_match[i] = (short)t;
      }
    }

    // 4, 5: update the matched slot, age the others
    bool is_free = own && !live;
    if (live) {
      if (mine >= 0) {
        const DetRow d = s_det[mine];
        float vx = s_vx[t], vy = s_vy[t];
        const float pt = s_pt[t];
        const int hits = s_hits[t];
        if (d.flags & kHasVel) {
          vx = d.vx;
          vy = d.vy;
        } else if (pt > 0.f) {
          const float vmx = (d.x - s_px[t]) / pt, vmy = (d.y - s_py[t]) / pt;
          if (hits == 1) {
            vx = vmx;
            vy = vmy;
          } else {
            vx = vx + alpha * (vmx - vx);
            vy = vy + alpha * (vmy - vy);
          }
        }
        s_vx[t] = vx; s_vy[t] = vy;
        s_x[t] = d.x; s_y[t] = d.y; s_px[t] = d.x; s_py[t] = d.y;
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

    // 6: births — the r-th unmatched valid detection takes the r-th free slot
    int n_free;
    const int fr = block_rank(is_free, s_cnt, &n_free);  // (its first barrier: s_match, s_id are written)
    if (is_free) s_free[fr] = (short)t;
    int born = 0;  // unmatched valid detections so far
    for (int i0 = 0; i0 < n; i0 += nt) {
      const int i = i0 + t;
      bool want = false, valid = false;
      if (i < n) {
        valid = (s_det[i].flags & kValid) != 0;
        want = valid && s_match[i] < 0;
      }
      int n_want;
      const int r = born + block_rank(want, s_cnt, &n_want);  // (its barriers: s_free is written)
      born += n_want;
      if (want && r < n_free) {
        const DetRow d = s_det[i];
        const int s = s_free[r];
        const bool has = (d.flags & kHasVel) != 0;
        const float vx = has ? d.vx : 0.f, vy = has ? d.vy : 0.f;
        s_id[s] = next_id + r;
        s_label[s] = d.label;
        s_x[s] = d.x; s_y[s] = d.y; s_px[s] = d.x; s_py[s] = d.y;
        s_vx[s] = vx; s_vy[s] = vy;
        s_pt[s] = 0.f;
        s_age[s] = 0;
        s_hits[s] = 1;
        out[n0 + i] = make_int4(next_id + r, 1, (int)__float_as_uint(vx), (int)__float_as_uint(vy));
      } else if (i < n && (!valid || want)) {
        out[n0 + i] = make_int4(0, 0, 0, 0);  // invalid, or no free slot
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

// rows: device, 32 B per detection (x, y, vx, vy float; label, flags int; 2 pad words), 16-byte aligned.
// det_off: HOST int[n_frames + 1], validated here and passed to the kernel by value.  dt float[n_frames],
// reset uint8[n_frames], max_dist2 float[n_gates] (the last entry: every label outside the table): device.
// state: device int[4 + 11 * capacity] (next_id, overflow, 2 pad; then id, label, x, y, vx, vy, px, py, pt, age,
// hits).  out: device int4 per detection (track id, hits, vx bits, vy bits).  Nothing is launched, and nothing
// written, on a bad argument.
TCA_API int tca_track3d(const void* rows, const int* det_off, int n_frames, const float* dt, const uint8_t* reset,
                        const float* max_dist2, int n_gates, int* state, int capacity, int max_age, float alpha,
                        void* out, hipStream_t stream) {
  if (capacity < 1 || capacity > kMaxCap || n_frames < 0 || n_frames > kMaxFrames || n_gates < 1 || max_age < 0)
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
      ((uintptr_t)dt & 3) != 0 || ((uintptr_t)max_dist2 & 3) != 0)
    return (int)hipErrorInvalidValue;
  if (n_frames == 0) return 0;
  if (dt == nullptr || reset == nullptr || max_dist2 == nullptr) return (int)hipErrorInvalidValue;
  if (offs.off[n_frames] > 0 && (rows == nullptr || out == nullptr)) return (int)hipErrorInvalidValue;
  const int threads = (capacity + kWave - 1) / kWave * kWave;
  track3d_kernel<<<1, threads, 0, stream>>>((const uint4*)rows, offs, n_frames, dt, reset, max_dist2, n_gates, state,
                                            capacity, max_age, alpha, (int4*)out);
  TCA_LAUNCH_CHECK();
}
