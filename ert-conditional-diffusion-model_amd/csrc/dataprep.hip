// Data preparation on device: the reference's scaling
// cell ERT_Conditional_Diffusion.py:230-269 and the inverse at :417-419.
//
//   MinMaxScaler.fit / partial_fit      data_min_ = nanmin(X, 0), data_max_ = nanmax(X, 0)
//                                        data_range_ = max - min
//                                        scale_ = (fr1 - fr0) / (range < 10 eps ? 1 : range)
//                                        min_   = fr0 - data_min_ * scale_
//   MinMaxScaler.transform               X *= scale_; X += min_          (float64, two roundings)
//   DiffusionDataset :72 + .float()      cond[i, c, l] = (float)scaled[i, l, c]
//   MinMaxScaler.inverse_transform       X -= min_; X /= scale_          (in X's dtype: a float32
//                                        array is rounded to float32 after each of the two ops)
//
// Every float64 operation is a separately rounded IEEE operation, so the
// results carry sklearn's bits.  All kernels stream HBM once; the yardstick
// is the copy rate, not the FLOP peak.
//
// Column statistics: lanes run along columns (two adjacent columns per lane
// through one 16-byte load where the row pitch allows), the rows are cut into
// slabs so the launch has a few thousand workgroups, each slab writes its
// column minima / maxima to the caller's workspace and a second kernel folds
// the slabs.  min / max are exact in any order: no atomics, and the result
// does not depend on the slab count.
//
// Condition build / inverse: one workgroup moves a tile of TL positions of one
// sample (the build: then the same tile of the next, RG samples in all, with
// the tile's scale_ / min_ values held in registers).  In the (n, L, C) layout the tile is one contiguous run of C * TL
// values; in the (n, C, L) layout it is C runs of TL floats.  The tile goes
// through LDS as tile[c][l] with an odd pitch (TL + 3) so that the side that
// walks c fastest spreads over the banks; both global sides are coalesced.
// The float rows of the (n, C, L) side start at 4-byte alignment only (odd L),
// so that side uses dword accesses: a wave still covers 256 contiguous bytes.
#include "ertd_common.h"

#include <cfloat>

#include "ertdiff.h"

namespace ertd {
namespace {

constexpr int DT = 256;              // threads per workgroup, every kernel here
constexpr int TL = 256;              // positions per condition tile
constexpr int TP = TL + 3;           // LDS pitch of one channel row (floats)
constexpr int CMAX = 16;             // most channels a condition tile holds
constexpr int RG = 8;                // samples one workgroup takes through the same tile
constexpr int SLAB_TARGET = 2048;    // workgroups the statistics launch aims for
constexpr int SLAB_MAX = 256;

inline int dp_rc(hipError_t e) { return e == hipSuccess ? ERTD_OK : (int)e; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// slabs of the statistics launch: a function of (n, F) alone, so that the
// workspace size does not depend on which load width the launch picks
inline int slab_count(long long n, long long F) {
  const long long cb = (F + 2 * DT - 1) / (2 * DT);
  long long s = (SLAB_TARGET + cb - 1) / cb;
  if (s > SLAB_MAX) s = SLAB_MAX;
  if (s > n) s = n;
  return (int)(s < 1 ? 1 : s);
}

// np.nanmin / np.nanmax step: fmin / fmax return the other operand when one is
// NaN, so a running value that starts as NaN stays NaN only for an all-NaN column
__device__ __forceinline__ void fold(double& mn, double& mx, double v) {
  mn = fmin(mn, v);
  mx = fmax(mx, v);
}

// Slab s of the rows, columns [W * (blockIdx.x * DT + tid), +W): partial
// min at part[s * F + col], partial max at part[(S + s) * F + col].
template <int W>
__global__ __launch_bounds__(DT) void colstats_kernel(const double* __restrict__ X, long long n,
                                                      long long F, long long ldx, int S,
                                                      double* __restrict__ part) {
  const long long col = ((long long)blockIdx.x * DT + threadIdx.x) * W;
  if (col >= F) return;
  const int s = blockIdx.y;
  const long long rows = (n + S - 1) / S;
  const long long r0 = (long long)s * rows;
  long long r1 = r0 + rows;
  if (r1 > n) r1 = n;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  double mn[W], mx[W];
#pragma unroll
  for (int w = 0; w < W; ++w) mn[w] = mx[w] = nan;
  const double* p = X + r0 * ldx + col;
  long long r = r0;
  if constexpr (W == 2) {
    // col is even and F is even (the launch picks W = 2 only then): col + 1 < F
    for (; r + 4 <= r1; r += 4, p += 4 * ldx) {
      const double2 a = *reinterpret_cast<const double2*>(p);
      const double2 b = *reinterpret_cast<const double2*>(p + ldx);
      const double2 c = *reinterpret_cast<const double2*>(p + 2 * ldx);
      const double2 d = *reinterpret_cast<const double2*>(p + 3 * ldx);
      fold(mn[0], mx[0], a.x); fold(mn[1], mx[1], a.y);
      fold(mn[0], mx[0], b.x); fold(mn[1], mx[1], b.y);
      fold(mn[0], mx[0], c.x); fold(mn[1], mx[1], c.y);
      fold(mn[0], mx[0], d.x); fold(mn[1], mx[1], d.y);
    }
    for (; r < r1; ++r, p += ldx) {
      const double2 a = *reinterpret_cast<const double2*>(p);
      fold(mn[0], mx[0], a.x); fold(mn[1], mx[1], a.y);
    }
  } else {
    for (; r + 4 <= r1; r += 4, p += 4 * ldx) {
      const double a = p[0], b = p[ldx], c = p[2 * ldx], d = p[3 * ldx];
      fold(mn[0], mx[0], a);
      fold(mn[0], mx[0], b);
      fold(mn[0], mx[0], c);
      fold(mn[0], mx[0], d);
    }
    for (; r < r1; ++r, p += ldx) fold(mn[0], mx[0], p[0]);
  }
#pragma unroll
  for (int w = 0; w < W; ++w) {
    part[(long long)s * F + col + w] = mn[w];
    part[((long long)S + s) * F + col + w] = mx[w];
  }
}

// Fold the S_used slabs of a column (a slab past the last row wrote nothing
// and is not read).  accumulate: then np.minimum / np.maximum with the stored
// value, as MinMaxScaler.partial_fit does -- those propagate a NaN.
__global__ __launch_bounds__(DT) void colstats_combine_kernel(const double* __restrict__ part, int S,
                                                              int S_used, long long F, int accumulate,
                                                              double* __restrict__ data_min,
                                                              double* __restrict__ data_max) {
  const long long col = (long long)blockIdx.x * DT + threadIdx.x;
  if (col >= F) return;
  double mn = part[col], mx = part[(long long)S * F + col];
  for (int s = 1; s < S_used; ++s) {
    mn = fmin(mn, part[(long long)s * F + col]);
    mx = fmax(mx, part[((long long)S + s) * F + col]);
  }
  if (accumulate) {
    const double pm = data_min[col], px = data_max[col];
    mn = (pm != pm || mn != mn) ? (pm != pm ? pm : mn) : (pm < mn ? pm : mn);
    mx = (px != px || mx != mx) ? (px != px ? px : mx) : (px > mx ? px : mx);
  }
  data_min[col] = mn;
  data_max[col] = mx;
}

__global__ __launch_bounds__(DT) void finalize_kernel(const double* __restrict__ data_min,
                                                      const double* __restrict__ data_max, long long F,
                                                      double fr0, double span,
                                                      double* __restrict__ scale, double* __restrict__ min_,
                                                      double* __restrict__ range) {
  const long long col = (long long)blockIdx.x * DT + threadIdx.x;
  if (col >= F) return;
  const double mn = data_min[col];
  const double rg = __dsub_rn(data_max[col], mn);
  // _handle_zeros_in_scale: scale[scale < 10 * eps] = 1.0 (a NaN compares false and stays)
  const double safe = (rg < 10.0 * DBL_EPSILON) ? 1.0 : rg;
  const double sc = __ddiv_rn(span, safe);
  scale[col] = sc;
  min_[col] = __dsub_rn(fr0, __dmul_rn(mn, sc));
  if (range) range[col] = rg;
}

__device__ __forceinline__ float scale_to_f32(double x, double sc, double mn) {
  return (float)__dadd_rn(__dmul_rn(x, sc), mn);
}
// float32 array under sklearn's in-place float64 operands: one rounding per op
__device__ __forceinline__ float unscale_f32(float x, double sc, double mn) {
  const float t = (float)__dsub_rn((double)x, mn);
  return (float)__ddiv_rn((double)t, sc);
}

// (n, L, C) float64 -> scaled (n, C, L) float32.  CT: the channel count when
// known at compile time (14), 0: read from C.  VEC: 16-byte loads of x,
// scale_ and min_ (C even and the three bases 16-byte aligned).
// A workgroup takes the same tile of RG consecutive samples and keeps the
// tile's scale_ / min_ values in registers across them: read per sample,
// they would pass 2 bytes through L2 for every byte of x from HBM.
template <int CT, bool VEC>
__global__ __launch_bounds__(DT) void cond_build_kernel(const double* __restrict__ X, long long n, int L,
                                                        int C_, int tiles,
                                                        const double* __restrict__ scale,
                                                        const double* __restrict__ min_,
                                                        float* __restrict__ cond) {
  __shared__ float tile[CMAX * TP];
  const int C = CT ? CT : C_;
  const long long g = blockIdx.x / tiles;
  const int l0 = (int)(blockIdx.x - g * tiles) * TL;
  const int tl = L - l0 < TL ? L - l0 : TL;
  const int cnt = tl * C;                         // values in this tile
  const long long f0 = (long long)l0 * C;         // feature index of the tile's first value
  const long long i0 = g * RG;
  const long long i1 = i0 + RG < n ? i0 + RG : n;
  constexpr int W = VEC ? 2 : 1;                  // values per lane and step
  constexpr int K = ((CT ? CT : CMAX) * TL / W + DT - 1) / DT;
  double s[K][W], m[K][W];
  int at[K][W];                                   // LDS slot of each value, -1 past the tile
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = W * (threadIdx.x + k * DT);     // VEC: cnt is even (C is), e + 1 < cnt
    const bool in = e < cnt;
    const int l = e / C, c = e - l * C;           // VEC: c even, so c + 1 < C at the same l
#pragma unroll
    for (int w = 0; w < W; ++w) {
      s[k][w] = in ? scale[f0 + e + w] : 0.0;
      m[k][w] = in ? min_[f0 + e + w] : 0.0;
      at[k][w] = in ? (c + w) * TP + l : -1;
    }
  }
  for (long long i = i0; i < i1; ++i) {
    const double* xp = X + i * (long long)L * C + f0;
    double x[K][W];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e = W * (threadIdx.x + k * DT);
      if constexpr (VEC) {
        const double2 v = e < cnt ? *reinterpret_cast<const double2*>(xp + e) : double2{0.0, 0.0};
        x[k][0] = v.x;
        x[k][1] = v.y;
      } else {
        x[k][0] = e < cnt ? xp[e] : 0.0;
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int w = 0; w < W; ++w)
        if (at[k][w] >= 0) tile[at[k][w]] = scale_to_f32(x[k][w], s[k][w], m[k][w]);
    __syncthreads();
    float* op = cond + i * (long long)C * L + l0;
    for (int o = threadIdx.x; o < C * TL; o += DT) {
      const int c = o / TL, l = o - c * TL;
      if (l < tl) op[(long long)c * L + l] = tile[c * TP + l];
    }
    __syncthreads();                              // the tile is rewritten for the next sample
  }
}

// (n, C, L) float32 -> unscaled (n, L, C) float32, the same tile backwards.
// One sample per workgroup: taking RG samples per workgroup with scale_ / min_
// in registers, as the build does, measured 1.46x slower here (1394 against
// 952 us at (5076, 14, 4693)) -- the float64 division and the LDS round trip
// then run one phase after the other in too few resident waves.
template <int CT>
__global__ __launch_bounds__(DT) void cond_inverse_kernel(const float* __restrict__ cond, int L, int C_,
                                                          int tiles, const double* __restrict__ scale,
                                                          const double* __restrict__ min_,
                                                          float* __restrict__ out) {
  __shared__ float tile[CMAX * TP];
  const int C = CT ? CT : C_;
  const long long i = blockIdx.x / tiles;
  const int l0 = (int)(blockIdx.x - i * tiles) * TL;
  const int tl = L - l0 < TL ? L - l0 : TL;
  const float* ip = cond + i * (long long)C * L + l0;
  for (int o = threadIdx.x; o < C * TL; o += DT) {
    const int c = o / TL, l = o - c * TL;
    if (l < tl) tile[c * TP + l] = ip[(long long)c * L + l];
  }
  __syncthreads();
  const int cnt = tl * C;
  const long long f0 = (long long)l0 * C;
  float* op = out + i * (long long)L * C + f0;
  for (int e = threadIdx.x; e < cnt; e += DT) {
    const int l = e / C, c = e - l * C;
    op[e] = unscale_f32(tile[c * TP + l], scale[f0 + e], min_[f0 + e]);
  }
}

// plain (n, F) transform / inverse: one element per thread, columns fastest
template <typename T, bool INVERSE>
__global__ __launch_bounds__(DT) void transform_kernel(const T* X, long long n, long long F,
                                                       long long ldx, const double* __restrict__ scale,
                                                       const double* __restrict__ min_, T* out,
                                                       long long ldo) {
  const long long idx = (long long)blockIdx.x * DT + threadIdx.x;
  if (idx >= n * F) return;
  const long long r = idx / F, c = idx - r * F;
  const T x = X[r * ldx + c];
  const double sc = scale[c], mn = min_[c];
  T y;
  if constexpr (INVERSE) {
    if constexpr (sizeof(T) == 4) y = unscale_f32(x, sc, mn);
    else y = __ddiv_rn(__dsub_rn(x, mn), sc);
  } else {
    y = __dadd_rn(__dmul_rn(x, sc), mn);
  }
  out[r * ldo + c] = y;
}

inline bool grid_ok(long long blocks) { return blocks >= 1 && blocks <= 0x7fffffffLL; }

}  // namespace
}  // namespace ertd

extern "C" {

using namespace ertd;

size_t ertd_minmax_ws_bytes(long long n, long long F) {
  if (n < 1 || F < 1) return 0;
  return (size_t)2 * slab_count(n, F) * (size_t)F * sizeof(double);
}

int ertd_minmax_partial_fit(const double* X, long long n, long long F, long long ldx,
                            double* data_min, double* data_max, int accumulate, void* ws,
                            size_t ws_bytes, void* stream) {
  if (!X || !data_min || !data_max || !ws || n < 1 || F < 1 || ldx < F) return ERTD_EINVAL;
  if (ws_bytes < ertd_minmax_ws_bytes(n, F)) return ERTD_ENOSPC;
  const hipStream_t s = (hipStream_t)stream;
  const int S = slab_count(n, F);
  const long long rows = (n + S - 1) / S;
  const int S_used = (int)((n + rows - 1) / rows);    // slabs that hold a row
  double* part = static_cast<double*>(ws);
  // 16-byte loads: every row start and every lane's pair must be 16-byte aligned
  const bool vec = F % 2 == 0 && ldx % 2 == 0 && aligned16(X);
  const long long cb = vec ? (F / 2 + DT - 1) / DT : (F + DT - 1) / DT;
  if (!grid_ok(cb)) return ERTD_EINVAL;
  const dim3 grid((unsigned)cb, (unsigned)S_used);
  if (vec) colstats_kernel<2><<<grid, DT, 0, s>>>(X, n, F, ldx, S, part);
  else colstats_kernel<1><<<grid, DT, 0, s>>>(X, n, F, ldx, S, part);
  colstats_combine_kernel<<<(unsigned)((F + DT - 1) / DT), DT, 0, s>>>(part, S, S_used, F, accumulate,
                                                                       data_min, data_max);
  return dp_rc(hipGetLastError());
}

int ertd_minmax_finalize(const double* data_min, const double* data_max, long long F, double fr0,
                         double fr1, double* scale, double* min_, double* range, void* stream) {
  if (!data_min || !data_max || !scale || !min_ || F < 1) return ERTD_EINVAL;
  const long long blocks = (F + DT - 1) / DT;
  if (!grid_ok(blocks)) return ERTD_EINVAL;
  finalize_kernel<<<(unsigned)blocks, DT, 0, (hipStream_t)stream>>>(data_min, data_max, F, fr0,
                                                                    fr1 - fr0, scale, min_, range);
  return dp_rc(hipGetLastError());
}

int ertd_minmax_transform(const double* X, long long n, long long F, long long ldx,
                          const double* scale, const double* min_, double* out, long long ldo,
                          void* stream) {
  if (!X || !scale || !min_ || !out || n < 1 || F < 1 || ldx < F || ldo < F) return ERTD_EINVAL;
  if (n > (1LL << 62) / F) return ERTD_EINVAL;
  const long long blocks = (n * F + DT - 1) / DT;
  if (!grid_ok(blocks)) return ERTD_EINVAL;
  transform_kernel<double, false><<<(unsigned)blocks, DT, 0, (hipStream_t)stream>>>(X, n, F, ldx, scale,
                                                                                    min_, out, ldo);
  return dp_rc(hipGetLastError());
}

int ertd_minmax_inverse(const void* X, int dtype, long long n, long long F, long long ldx,
                        const double* scale, const double* min_, void* out, long long ldo,
                        void* stream) {
  if (!X || !scale || !min_ || !out || n < 1 || F < 1 || ldx < F || ldo < F) return ERTD_EINVAL;
  if (dtype != ERTD_F32 && dtype != ERTD_F64) return ERTD_EINVAL;
  if (n > (1LL << 62) / F) return ERTD_EINVAL;
  const long long blocks = (n * F + DT - 1) / DT;
  if (!grid_ok(blocks)) return ERTD_EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  if (dtype == ERTD_F32)
    transform_kernel<float, true><<<(unsigned)blocks, DT, 0, s>>>(
        static_cast<const float*>(X), n, F, ldx, scale, min_, static_cast<float*>(out), ldo);
  else
    transform_kernel<double, true><<<(unsigned)blocks, DT, 0, s>>>(
        static_cast<const double*>(X), n, F, ldx, scale, min_, static_cast<double*>(out), ldo);
  return dp_rc(hipGetLastError());
}

int ertd_minmax_cond(const double* X, long long n, int L, int C, const double* scale,
                     const double* min_, float* cond, void* stream) {
  if (!X || !scale || !min_ || !cond || n < 1 || L < 1 || C < 1 || C > CMAX) return ERTD_EINVAL;
  const int tiles = (L + TL - 1) / TL;
  if (n > 0x7fffffffLL) return ERTD_EINVAL;
  const long long blocks = (n + RG - 1) / RG * tiles;
  if (!grid_ok(blocks)) return ERTD_EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  const unsigned g = (unsigned)blocks;
  // C even: every tile starts a multiple of 16 bytes into X
  const bool vec = C % 2 == 0 && aligned16(X);
  if (C == CIN && vec) cond_build_kernel<CIN, true><<<g, DT, 0, s>>>(X, n, L, C, tiles, scale, min_, cond);
  else if (vec) cond_build_kernel<0, true><<<g, DT, 0, s>>>(X, n, L, C, tiles, scale, min_, cond);
  else cond_build_kernel<0, false><<<g, DT, 0, s>>>(X, n, L, C, tiles, scale, min_, cond);
  return dp_rc(hipGetLastError());
}

int ertd_minmax_cond_inverse(const float* cond, long long n, int L, int C, const double* scale,
                             const double* min_, float* out, void* stream) {
  if (!cond || !scale || !min_ || !out || n < 1 || L < 1 || C < 1 || C > CMAX) return ERTD_EINVAL;
  const int tiles = (L + TL - 1) / TL;
  if (n > 0x7fffffffLL) return ERTD_EINVAL;
  const long long blocks = n * tiles;
  if (!grid_ok(blocks)) return ERTD_EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  const unsigned g = (unsigned)blocks;
  if (C == CIN) cond_inverse_kernel<CIN><<<g, DT, 0, s>>>(cond, L, C, tiles, scale, min_, out);
  else cond_inverse_kernel<0><<<g, DT, 0, s>>>(cond, L, C, tiles, scale, min_, out);
  return dp_rc(hipGetLastError());
}

}  // extern "C"
