// What K35 (voxel_normals.hip) and K36 (voxel_outliers.hip) share: the cell lists of a fixed-radius neighbour search
// over the records of tca_voxel_downsample, built in the bytes of its dead leaf table.
//
//     cells   16 bytes a slot, slots[b] per cloud: key int64 | count int32 | start int32, open addressing, linear
//             probing; the key packs the three cell indices (21 bits each), -1 is empty.  A cell has the side R and its
//             index is the FLOOR of q / R (-1 and +1 lie in different cells), so every neighbour of a voxel lies in
//             the 27 cells around its own, exactly.
//     sorted  16 bytes a record, the cloud's records one cell after the other: qx, qy, qz, row.
//     zeroed  int32s behind them: the cursor of every cloud last, whatever else the caller wants cleared in front.
//
//   reset   every cell slot empty, every zeroed int 0.
//   keys    a row claims its cell's slot (one 64-bit compare-and-swap); its atomicAdd on the slot's count is its rank
//           inside the cell.  (slot, rank) wait in 16 bytes of scratch at the row's index.
//   starts  every slot takes its cell's first record from the cloud's cursor: a wave adds its 64 counts with shuffles
//           and advances the cursor once.  A per-cloud prefix in slot order would do the same with one workgroup
//           walking slots[b] slots; the cursor spreads that over the device at the price of an order of the cells that
//           depends on who won the atomics, like the order inside a cell.
//   sort    a row stores its quad at start + rank.
//
// Every kernel here has internal linkage: each file that includes the header carries its own copy.
#pragma once
#include "tca_common.h"

namespace tca {

constexpr int kCellBlock = 256;
constexpr int kCellFrames = 64;
constexpr int kCellPoints = 1 << 24;
constexpr int kCellBias = 1 << 20;
constexpr int kCellMaxRadius = 4 << 16;
constexpr unsigned long long kEmptyCell = ~0ull;

struct Cell {  // 16 bytes
  unsigned long long key;
  int count, start;
};
static_assert(sizeof(Cell) == 16, "a cell slot is 16 bytes");

struct CellArgs {
  int radius;                  // R, units of 2^-16 m
  int max_n;
  int n[kCellFrames];          // the points of cloud b the host knows: the most records it has
  int pt_off[kCellFrames];     // the records before cloud b's
  int mask[kCellFrames];       // slots[b] - 1
  long slot_off[kCellFrames];  // the slots before cloud b's
};

__device__ __forceinline__ int records_of(const int* __restrict__ counts, const CellArgs& a, int b) {
  return min(max(counts[b], 0), a.n[b]);
}

__device__ __forceinline__ int quantise(unsigned bits) {
  const float v = __uint_as_float(bits);
  return fabsf(v) <= 512.f ? (int)rintf(v * 65536.f) : 0;  // (a record of tca_voxel_downsample always is)
}

__device__ __forceinline__ int floor_div(int q, int r) {
  const int d = q / r;
  return (q % r != 0 && q < 0) ? d - 1 : d;
}

__device__ __forceinline__ unsigned long long cell_key(int cx, int cy, int cz) {
  return ((unsigned long long)(cz + kCellBias) << 42) | ((unsigned long long)(cy + kCellBias) << 21) |
         (unsigned long long)(cx + kCellBias);
}

__device__ __forceinline__ unsigned hash_of(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (unsigned)k;
}

// The records of cell `key`: where they start and how many, 0 if the cell is empty or the run is not inside [0, K).
__device__ __forceinline__ int find_cell(const Cell* __restrict__ tab, int mask, unsigned long long key, int K,
                                         int* start) {
  unsigned h = hash_of(key) & (unsigned)mask;
  for (int probe = 0; probe <= mask; ++probe, h = (h + 1u) & (unsigned)mask) {
    const unsigned long long seen = tab[h].key;
    if (seen == kEmptyCell) return 0;
    if (seen == key) {
      const int s = tab[h].start, n = tab[h].count;
      *start = s;
      return (s >= 0 && n > 0 && n <= K && s <= K - n) ? n : 0;
    }
  }
  return 0;
}

static __global__ void __launch_bounds__(kCellBlock) cells_reset_kernel(uint4* __restrict__ cells, long n_slots,
                                                                        int* __restrict__ zeroed, int n_zeroed) {
  const long i = (long)blockIdx.x * kCellBlock + threadIdx.x;
  if (i < n_slots) cells[i] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);
  else if (i < n_slots + n_zeroed) zeroed[i - n_slots] = 0;
}

static __global__ void __launch_bounds__(kCellBlock) cells_keys_kernel(const uint4* __restrict__ rows,
                                                                       const int* __restrict__ counts, CellArgs a,
                                                                       Cell* __restrict__ cells,
                                                                       uint4* __restrict__ scratch) {
  const int b = blockIdx.y;
  const int K = records_of(counts, a, b);
  const long i = (long)blockIdx.x * kCellBlock + threadIdx.x;
  if (i >= K) return;
  const uint4 rec = rows[a.pt_off[b] + i];
  const unsigned long long key = cell_key(floor_div(quantise(rec.x), a.radius), floor_div(quantise(rec.y), a.radius),
                                          floor_div(quantise(rec.z), a.radius));
  Cell* tab = cells + a.slot_off[b];
  const int mask = a.mask[b];
  int slot = -1, rank = 0;
  unsigned h = hash_of(key) & (unsigned)mask;
  // at most K <= slots[b] distinct cells: the probe ends at the key or at an empty slot
  for (int probe = 0; probe <= mask; ++probe, h = (h + 1u) & (unsigned)mask) {
    unsigned long long seen = tab[h].key;  // (a key never changes once it is set)
    if (seen == kEmptyCell) seen = atomicCAS(&tab[h].key, kEmptyCell, key);
    if (seen == kEmptyCell || seen == key) {
      slot = (int)h;
      rank = atomicAdd(&tab[h].count, 1);
      break;
    }
  }
  scratch[a.pt_off[b] + i] = make_uint4((unsigned)slot, (unsigned)rank, 0u, 0u);
}

static __global__ void __launch_bounds__(kCellBlock) cells_starts_kernel(CellArgs a, Cell* __restrict__ cells,
                                                                         int* __restrict__ cursor) {
  const int b = blockIdx.y;
  const long s = (long)blockIdx.x * kCellBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool in = s <= a.mask[b];
  Cell* tab = cells + a.slot_off[b];
  const int own = in ? tab[s].count : 0;
  int upto = own;  // the wave's inclusive prefix (every lane of the wave is here: no early return above)
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(upto, o, 64);
    if (lane >= o) upto += t;
  }
  int base = 0;
  if (lane == 63 && upto > 0) base = atomicAdd(&cursor[b], upto);
  base = __shfl(base, 63, 64);
  if (in) tab[s].start = base + upto - own;
}

static __global__ void __launch_bounds__(kCellBlock) cells_sort_kernel(const uint4* __restrict__ rows,
                                                                       const int* __restrict__ counts, CellArgs a,
                                                                       const Cell* __restrict__ cells,
                                                                       const uint4* __restrict__ scratch,
                                                                       int4* __restrict__ sorted) {
  const int b = blockIdx.y;
  const int K = records_of(counts, a, b);
  const long i = (long)blockIdx.x * kCellBlock + threadIdx.x;
  if (i >= K) return;
  const uint4 rec = rows[a.pt_off[b] + i];
  const uint4 sr = scratch[a.pt_off[b] + i];
  const int slot = (int)sr.x, rank = (int)sr.y;
  if (slot < 0 || slot > a.mask[b] || rank < 0) return;  // (never: the keys pass wrote it)
  const long pos = (long)cells[a.slot_off[b] + slot].start + rank;
  if (pos >= 0 && pos < K) sorted[a.pt_off[b] + pos] = make_int4(quantise(rec.x), quantise(rec.y), quantise(rec.z), (int)i);
}

// What a launch works on: the sums over the clouds and where its parts of the table lie.
struct CellPlan {
  CellArgs a;
  long n_sum, slot_sum;
  int max_slots;
  Cell* cells;
  int4* sorted;
  int* zeroed;  // n_zeroed int32s behind the sorted records, the clouds' cursors the last `batch` of them
  int* cursor;
};

// ns, slots: HOST int[B], what tca_voxel_downsample took; front: the int32s the caller wants cleared in front of the
// cursors.  False where a size is out of range or the parts do not fit the leaf table's 48 bytes a slot.
inline bool cell_plan(const int* ns, const int* slots, int batch, int radius_q, int front, void* table, long table_bytes,
                      CellPlan& p) {
  if (batch < 1 || batch > kCellFrames || ns == nullptr || slots == nullptr || radius_q < 1 || radius_q > kCellMaxRadius)
    return false;
  p.n_sum = p.slot_sum = 0;
  p.max_slots = 0;
  int max_n = 0;
  for (int b = 0; b < batch; ++b) {
    const int n = ns[b], s = slots[b];
    if (n < 0 || n > kCellPoints || s < 2 || s < n || (s & (s - 1)) != 0) return false;
    p.a.n[b] = n;
    p.a.mask[b] = s - 1;
    p.a.pt_off[b] = (int)p.n_sum;
    p.a.slot_off[b] = p.slot_sum;
    p.n_sum += n;
    p.slot_sum += s;
    max_n = n > max_n ? n : max_n;
    p.max_slots = s > p.max_slots ? s : p.max_slots;
    if (p.n_sum >= 0x80000000L / 16) return false;
  }
  // cells, sorted and the zeroed ints fit the leaf table: 16 (slots + n) + 4 (B + front) <= 32 slots + 4 front
  if (front < 0 || front > 7 * batch || table_bytes < 48 * p.slot_sum || table == nullptr || ((uintptr_t)table & 15) != 0)
    return false;
  p.a.radius = radius_q;
  p.a.max_n = max_n;
  p.cells = (Cell*)table;
  p.sorted = (int4*)((uint8_t*)table + 16 * p.slot_sum);
  p.zeroed = (int*)((uint8_t*)table + 16 * (p.slot_sum + p.n_sum));
  p.cursor = p.zeroed + front;
  return true;
}

// reset, keys, starts, sort on `stream`: rows' records (counts[b] of cloud b) into the plan's cells and sorted.
inline int cell_lists_build(const CellPlan& p, const uint4* rows, const int* counts, int batch, int front, uint4* scratch,
                            hipStream_t stream) {
  const int nblk = (p.a.max_n + kCellBlock - 1) / kCellBlock;
  const int n_zeroed = front + batch;
  cells_reset_kernel<<<(unsigned)((p.slot_sum + n_zeroed + kCellBlock - 1) / kCellBlock), kCellBlock, 0, stream>>>(
      (uint4*)p.cells, p.slot_sum, p.zeroed, n_zeroed);
  if (int e = (int)hipGetLastError()) return e;
  cells_keys_kernel<<<dim3(nblk, batch), kCellBlock, 0, stream>>>(rows, counts, p.a, p.cells, scratch);
  if (int e = (int)hipGetLastError()) return e;
  cells_starts_kernel<<<dim3((p.max_slots + kCellBlock - 1) / kCellBlock, batch), kCellBlock, 0, stream>>>(p.a, p.cells,
                                                                                                          p.cursor);
  if (int e = (int)hipGetLastError()) return e;
  cells_sort_kernel<<<dim3(nblk, batch), kCellBlock, 0, stream>>>(rows, counts, p.a, p.cells, scratch, p.sorted);
  return (int)hipGetLastError();
}

}  // namespace tca
