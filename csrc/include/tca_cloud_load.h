// Reading a point's FLOAT32 fields out of raw PointCloud2 bytes in place: the three load
// paths of K22 (points in boxes) and K23 (bird's-eye view), as a header for K26 (camera
// ranging), K27 (depth image) and later kernels.  K22 and K23 keep their own text of the same statements: calling
// these helpers instead changes their register allocation, and their code objects are to stay
// as they are.
//
// The launcher classifies the layout once (cloud_fast_path): 2 when the fields are the dwords
// at 0 / 4 / 8 (/ 12) of a record whose step is a multiple of 16 and the base pointer is 16-B
// aligned (one 16-B load per point), 1 when offsets, step and base pointer are 4-B aligned
// (dword loads), 0 otherwise (byte loads).  A frame's byte offset must be as aligned:
// cloud_frame_path lowers the path per frame.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tca {

__device__ __forceinline__ uint32_t load_u32_bytes(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

__device__ __forceinline__ int cloud_frame_path(int fast, long foff) {
  return (fast == 2 && (foff & 15) == 0) ? 2 : (fast >= 1 && (foff & 3) == 0) ? 1 : 0;
}

// raw[f] = the dword at rec + off[f] for every off[f] >= 0 (the others keep their value).
__device__ __forceinline__ void cloud_load_fields(const uint8_t* rec, const int (&off)[4], int fast,
                                                  uint32_t (&raw)[4]) {
  if (fast == 2) {
    const uint4 q = *reinterpret_cast<const uint4*>(rec);
    raw[0] = q.x; raw[1] = q.y; raw[2] = q.z; raw[3] = q.w;
  } else if (fast == 1) {
#pragma unroll
    for (int f = 0; f < 4; ++f)
      if (off[f] >= 0) raw[f] = *reinterpret_cast<const uint32_t*>(rec + off[f]);
  } else {
#pragma unroll
    for (int f = 0; f < 4; ++f)
      if (off[f] >= 0) raw[f] = load_u32_bytes(rec + off[f]);
  }
}

// Host: the layout's path, -1 for a field outside the record.  off[3] == -1: no fourth field;
// path 2 needs the fourth field at byte 12, or, with `fourth_optional`, at 12 or absent.
inline int cloud_fast_path(const void* data, int point_step, const int (&off)[4], bool fourth_optional) {
  bool dword = (point_step & 3) == 0 && ((uintptr_t)data & 3) == 0;
  for (int f = 0; f < 4; ++f) {
    const int o = off[f];
    if (f == 3 && o == -1) continue;
    if (o < 0 || o + 4 > point_step) return -1;
    dword = dword && (o & 3) == 0;
  }
  if (!dword) return 0;
  const bool fourth = off[3] == 12 || (fourth_optional && off[3] == -1);
  return (off[0] == 0 && off[1] == 4 && off[2] == 8 && fourth && (point_step & 15) == 0 &&
          ((uintptr_t)data & 15) == 0) ? 2 : 1;
}

}  // namespace tca
