// Medians of 9 and of 25 keys as fixed compare-exchange networks on an array the compiler keeps in registers
// (every index is a constant).  The exchange lists are N. Devillard's opt_med9 and opt_med25 ("Fast median search:
// an ANSI C implementation", 1998, public domain; the 9 is Paeth's from Graphics Gems): 19 and 99 exchanges, the
// fewest known.  p is left partly sorted.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define TCA_HD __host__ __device__ __forceinline__
#else
#define TCA_HD inline
#endif

namespace tca {

template <typename T> TCA_HD void median_cx(T& a, T& b) {
  const T lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

#define TCA_CX(i, j) median_cx(p[i], p[j])

template <typename T> TCA_HD T median9(T* p) {
  TCA_CX(1, 2); TCA_CX(4, 5); TCA_CX(7, 8); TCA_CX(0, 1); TCA_CX(3, 4); TCA_CX(6, 7);
  TCA_CX(1, 2); TCA_CX(4, 5); TCA_CX(7, 8); TCA_CX(0, 3); TCA_CX(5, 8); TCA_CX(4, 7);
  TCA_CX(3, 6); TCA_CX(1, 4); TCA_CX(2, 5); TCA_CX(4, 7); TCA_CX(4, 2); TCA_CX(6, 4);
  TCA_CX(4, 2);
  return p[4];
}

template <typename T> TCA_HD T median25(T* p) {
  TCA_CX(0, 1); TCA_CX(3, 4); TCA_CX(2, 4); TCA_CX(2, 3); TCA_CX(6, 7); TCA_CX(5, 7);
  TCA_CX(5, 6); TCA_CX(9, 10); TCA_CX(8, 10); TCA_CX(8, 9); TCA_CX(12, 13); TCA_CX(11, 13);
  TCA_CX(11, 12); TCA_CX(15, 16); TCA_CX(14, 16); TCA_CX(14, 15); TCA_CX(18, 19); TCA_CX(17, 19);
  TCA_CX(17, 18); TCA_CX(21, 22); TCA_CX(20, 22); TCA_CX(20, 21); TCA_CX(23, 24); TCA_CX(2, 5);
  TCA_CX(3, 6); TCA_CX(0, 6); TCA_CX(0, 3); TCA_CX(4, 7); TCA_CX(1, 7); TCA_CX(1, 4);
  TCA_CX(11, 14); TCA_CX(8, 14); TCA_CX(8, 11); TCA_CX(12, 15); TCA_CX(9, 15); TCA_CX(9, 12);
  TCA_CX(13, 16); TCA_CX(10, 16); TCA_CX(10, 13); TCA_CX(20, 23); TCA_CX(17, 23); TCA_CX(17, 20);
  TCA_CX(21, 24); TCA_CX(18, 24); TCA_CX(18, 21); TCA_CX(19, 22); TCA_CX(8, 17); TCA_CX(9, 18);
  TCA_CX(0, 18); TCA_CX(0, 9); TCA_CX(10, 19); TCA_CX(1, 19); TCA_CX(1, 10); TCA_CX(11, 20);
  TCA_CX(2, 20); TCA_CX(2, 11); TCA_CX(12, 21); TCA_CX(3, 21); TCA_CX(3, 12); TCA_CX(13, 22);
  TCA_CX(4, 22); TCA_CX(4, 13); TCA_CX(14, 23); TCA_CX(5, 23); TCA_CX(5, 14); TCA_CX(15, 24);
  TCA_CX(6, 24); TCA_CX(6, 15); TCA_CX(7, 16); TCA_CX(7, 19); TCA_CX(13, 21); TCA_CX(15, 23);
  TCA_CX(7, 13); TCA_CX(7, 15); TCA_CX(1, 9); TCA_CX(3, 11); TCA_CX(5, 17); TCA_CX(11, 17);
  TCA_CX(9, 17); TCA_CX(4, 10); TCA_CX(6, 12); TCA_CX(7, 14); TCA_CX(4, 6); TCA_CX(4, 7);
  TCA_CX(12, 14); TCA_CX(10, 14); TCA_CX(6, 7); TCA_CX(10, 12); TCA_CX(6, 10); TCA_CX(6, 17);
  TCA_CX(12, 17); TCA_CX(7, 17); TCA_CX(7, 10); TCA_CX(12, 18); TCA_CX(7, 12); TCA_CX(10, 18);
  TCA_CX(12, 20); TCA_CX(10, 20); TCA_CX(10, 12);
  return p[12];
}

#undef TCA_CX

}  // namespace tca
