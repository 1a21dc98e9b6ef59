// What K31 (cluster.hip) and K32 (cluster_fit.hip) share: a row of the cluster table and the runs of a wave.
#pragma once
#include <hip/hip_runtime.h>

namespace tca {

struct Row {  // 64 bytes: ops/cluster.py TABLE_DTYPE
  int n, root;
  int min_x, max_x, min_y, max_y, min_z, max_z;
  long long sum_x, sum_y, sum_z, pad;
};
static_assert(sizeof(Row) == 64, "a table row is 64 bytes");

// The run of consecutive lanes with this lane's key (key < 0: no run): is the lane its head, its position in
// the run and the run's length.
struct Run {
  bool head;
  int pos, len;
};

__device__ __forceinline__ Run wave_run(int key) {
  const int lane = threadIdx.x & 63;
  const int prev = __shfl_up(key, 1, 64);
  Run r;
  r.head = key >= 0 && (lane == 0 || prev != key);
  const unsigned long long brk = __ballot(key < 0 || r.head);  // every run starts at a break
  const unsigned long long after = lane == 63 ? 0ull : (brk >> (lane + 1));
  const int rest = after ? (__builtin_ctzll(after) + 1) : (64 - lane);  // lanes from this one to the run's end
  const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
  r.pos = (brk & upto) ? lane - (63 - __builtin_clzll(brk & upto)) : 0;
  r.len = r.pos + rest;
  return r;
}

}  // namespace tca
