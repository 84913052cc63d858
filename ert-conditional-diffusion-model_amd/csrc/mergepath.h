// Merge-path partition arithmetic of the row sort and the Wasserstein walk
// (csrc/rowsort.hip).  Host and device: every index a kernel forms from a
// diagonal comes out of these functions, so a host program can enumerate
// them (tools/mergepath_check.cpp) before a kernel ever runs.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ERTD_MP_HD __host__ __device__ __forceinline__
#else
#define ERTD_MP_HD inline
#endif

namespace ertd {
namespace mp {

// np.sort's order: ascending, every NaN after every number, NaNs tied.
template <typename T>
ERTD_MP_HD bool key_less(T a, T b) {
  return a < b || (b != b && a == a);
}

// The stable merge of sorted A (la keys) and B (lb keys) takes A on ties.
// Returns how many of its first d keys (0 <= d <= la + lb) come from A; the
// other d - a come from B.  Reads A[mid] and B[d - 1 - mid] only with
// max(0, d - lb) <= mid < min(d, la), so both indices are inside their runs.
template <typename T>
ERTD_MP_HD long long merge_path(const T* A, long long la, const T* B, long long lb, long long d) {
  long long lo = d - lb > 0 ? d - lb : 0;
  long long hi = d < la ? d : la;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (key_less(B[d - 1 - mid], A[mid])) hi = mid;   // A[mid] comes after B[d-1-mid]
    else lo = mid + 1;
  }
  return lo;
}

// One step of the serial merge: true when the next key comes from A.
// ai <= la and bi <= lb, not both at their ends; a run at its end is not read.
template <typename T>
ERTD_MP_HD bool take_a(const T* A, long long la, long long ai, const T* B, long long lb,
                       long long bi) {
  if (bi >= lb) return true;
  if (ai >= la) return false;
  return !key_less(B[bi], A[ai]);
}

// Sorted runs of a row of M keys before merge pass p have length L = tile << p
// (the last one shorter).  The output position pos of pass p lies in the merged
// run R = pos / 2L, made of runs 2R (a0, la >= 1) and 2R + 1 (b0, lb >= 0: an
// odd run at the end of a pass is copied through); d is pos's diagonal in it.
struct RunPair {
  long long a0, la, b0, lb, d;
};

ERTD_MP_HD RunPair run_pair(long long M, long long L, long long pos) {
  RunPair r;
  const long long R = pos / (2 * L);
  r.a0 = 2 * R * L;
  r.b0 = r.a0 + L;
  const long long end = r.b0 + L < M ? r.b0 + L : M;
  r.la = r.b0 < M ? L : M - r.a0;
  r.lb = r.b0 < M ? end - r.b0 : 0;
  if (r.b0 > M) r.b0 = M;
  r.d = pos - r.a0;
  return r;
}

ERTD_MP_HD long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// merge passes that turn `runs` sorted runs into one
ERTD_MP_HD int merge_passes(long long runs) {
  int p = 0;
  while (((long long)1 << p) < runs) ++p;
  return p;
}

}  // namespace mp
}  // namespace ertd
