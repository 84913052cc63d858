// Ensemble order statistics, coverage calibration, moments and WSSE on the
// device (ertdiff/stats.py).
//
// Reference: ERT_Conditional_Diffusion.py
//   :867-876   np.mean / np.std / np.var / np.percentile(sim_data, 25|50|75, axis=0)
//   :1121-1132 the calibration loop: 60 np.percentile calls over the realisation
//              axis of Uncertainty_params (S, N, 29), the coverage indicator
//              (low < true) & (true <= upp) and its mean per level
//   :767-787   WSSE per realisation and survey
//
// Percentiles are numpy's method="linear" operation for operation
// (numpy/lib/_function_base_impl.py _quantile / _lerp), on the sorted column s
// of m used samples and a float64 fraction q:
//   vi = (m-1)*q   lo = floor(vi)   hi = min(lo+1, m-1)   t = vi - lo
//   d  = s[hi] - s[lo]              (in the input's dtype, then promoted)
//   r  = t < 0.5 ? s[lo] + d*t : s[hi] - d*(1-t)          (float64)
// so the result carries np.percentile's bits.  A NaN among the used samples
// makes every percentile of the column NaN (numpy sorts it last and checks).
//
// Sort: one 256-thread workgroup stages a tile of tc adjacent columns x npad
// rows in LDS (npad = n rounded up to a power of two, at least 64; the tail
// and the masked samples filled with +inf), adjacent lanes loading adjacent
// columns while the tile walks the rows; column pitch npad+1 keeps the
// transposing stores off one bank.  A bitonic network (uniform control flow)
// then sorts every column:
//   n <= 256   a wave takes a column into registers (64 keys per register),
//              exchanges across lanes, and writes it back sorted -- the
//              calibration's S = 50 and the simulated ensemble's n = 100;
//   n >  256   the network runs in LDS over the whole tile at once: the
//              tc*npad/2 compare-exchanges of a stage are a flat index space
//              strided over the threads, many columns per workgroup or one
//              long column across it (n = 16384: 128 KiB of float64 keys).
// Keys stay in the input dtype; only the two order statistics a percentile
// selects are promoted.
#include "ertd_common.h"

#include <cmath>

#include "ertdiff.h"

namespace ertd {
namespace {

constexpr int ET = 256;                   // threads per workgroup
constexpr int TILE_BYTES = 32 * 1024;     // key tile budget of the many-column regime
constexpr int MAX_N = 16384;              // 128 KiB of float64 keys
constexpr int MAX_LDS = 160 * 1024;
constexpr int SU = 8;                     // row loads in flight per thread while staging
constexpr int MAX_WAVE_R = 4;             // columns of up to 256 keys are sorted in registers
constexpr int MAX_CNT = 4096;             // (K + 1) * P coverage counters in LDS

struct TileArgs {
  const void* x;            // (n, ld) row-major, column c < cells
  int n;
  long long cells, ld;
  const uint8_t* valid;     // (n, vcols) or null; entry covers rpv adjacent columns
  long long vcols;
  int rpv;
  int npad, lognp, tc, logtc, ldk;
  int wave_r;               // > 0: npad = 64 * wave_r keys per column, sorted in one wave's registers
  // percentiles
  const double* q;          // (nq) fractions in [0, 1]
  int nq;
  double* out;              // (nq, cells)
  int* n_eff;               // (cells) or null
  // coverage
  const void* truth;        // (cells), the input's dtype
  const double* q_low;      // (K)
  const double* q_upp;      // (K)
  int K, P;
  int* counts;              // (K, P)
  int* cols;                // (P)
};

template <typename T>
__device__ __forceinline__ double lerp_quantile(const T* s, int m, double q) {
  const double vi = (double)(m - 1) * q;
  const double fl = floor(vi);
  int lo = (int)fl;
  lo = lo < 0 ? 0 : (lo > m - 1 ? m - 1 : lo);
  const int hi = lo + 1 < m ? lo + 1 : m - 1;
  const double t = vi - fl;
  const T a = s[lo], b = s[hi];
  const T d = b - a;
  const double dd = (double)d;
  return t < 0.5 ? (double)a + dd * t : (double)b - dd * (1.0 - t);
}

// Short columns (npad = 64 R <= 256): one wave sorts a column in registers.
// Key i = 64 r + lane lives in v[r] of that lane; a stage of stride j < 64 is
// one cross-lane exchange (lane ^ j) per key, a stage of stride >= 64 a
// compare-exchange between two registers of the lane.  The four waves take
// the tile's columns in turn; no workgroup barrier inside the network.
template <typename T, int R>
__device__ __forceinline__ void wave_sort_columns(T* keys, int tc, int ldk, int tid) {
  const int lane = tid & 63;
  for (int col = tid >> 6; col < tc; col += ET / 64) {
    T* kc = keys + (size_t)col * ldk;
    T v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = kc[r * 64 + lane];
    for (int k = 2; k <= 64 * R; k <<= 1) {
#pragma unroll
      for (int jr = R / 2; jr >= 1; jr >>= 1) {   // strides 64 jr <= k / 2, largest first
        if ((jr << 6) < k) {
#pragma unroll
          for (int r = 0; r < R; ++r)
            if ((r & jr) == 0) {
              const bool asc = (((r << 6) | lane) & k) == 0;
              const T u = v[r], w = v[r | jr];
              const bool sw = (u > w) == asc;
              v[r] = sw ? w : u;
              v[r | jr] = sw ? u : w;
            }
        }
      }
      for (int j = (k >> 1) < 32 ? (k >> 1) : 32; j > 0; j >>= 1) {
        const bool lower = (lane & j) == 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const bool asc = (((r << 6) | lane) & k) == 0;
          const T u = v[r];
          const T w = __shfl_xor(u, j);
          v[r] = (lower == asc) ? (w < u ? w : u) : (w > u ? w : u);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) kc[r * 64 + lane] = v[r];
  }
}

// COVER = false: percentiles of every column; true: the fused calibration loop.
template <typename T, bool COVER>
__global__ __launch_bounds__(ET) void ens_tile_kernel(TileArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int tc = a.tc, npad = a.npad, ldk = a.ldk, n = a.n;
  T* keys = reinterpret_cast<T*>(smem);
  const size_t key_bytes = (((size_t)tc * ldk * sizeof(T)) + 15) & ~(size_t)15;
  int* ms = reinterpret_cast<int*>(smem + key_bytes);   // used samples per column
  int* nanf = ms + tc;                                  // column holds a NaN
  int* cnt = nanf + tc;                                 // COVER: (K, P) hits, then (P) columns
  const long long c0 = (long long)blockIdx.x * tc;
  const T* __restrict__ x = static_cast<const T*>(a.x);

  for (int i = tid; i < tc; i += ET) {
    ms[i] = (!a.valid && c0 + i < a.cells) ? n : 0;
    nanf[i] = 0;
  }
  if (COVER)
    for (int i = tid; i < (a.K + 1) * a.P; i += ET) cnt[i] = 0;
  __syncthreads();

  // stage: lane -> column, the loop walks the rows (coalesced), LDS is
  // column-major.  A thread keeps one column (tc <= 256 divides the block) and
  // issues SU row loads before it touches LDS; addresses are clamped into the
  // array and the value selected afterwards, so the loads carry no branch.
  {
    const int col = tid & (tc - 1);
    const int row0 = tid >> a.logtc, rstep = ET >> a.logtc;
    const long long c = c0 + col;
    const bool cin = c < a.cells;
    const long long cc = cin ? c : a.cells - 1;
    const uint8_t* vp = a.valid ? a.valid + cc / a.rpv : nullptr;
    const T* xp = x + cc;
    T* kc = keys + (size_t)col * ldk;
    int used = 0;
    bool has_nan = false;
    for (int rb = row0; rb < npad; rb += SU * rstep) {
      T v[SU];
      bool use[SU];
#pragma unroll
      for (int u = 0; u < SU; ++u) {
        const int row = rb + u * rstep;
        const int rc = row < n ? row : n - 1;
        use[u] = cin && row < n;
        if (vp) use[u] = use[u] && vp[(long long)rc * a.vcols] != 0;
        v[u] = xp[(long long)rc * a.ld];
      }
#pragma unroll
      for (int u = 0; u < SU; ++u) {
        const int row = rb + u * rstep;
        T w = use[u] ? v[u] : (T)INFINITY;
        used += use[u] ? 1 : 0;
        if (w != w) {
          has_nan = true;
          w = (T)INFINITY;
        }
        if (row < npad) kc[row] = w;
      }
    }
    if (a.valid && used) atomicAdd(&ms[col], used);
    if (has_nan) nanf[col] = 1;
  }
  __syncthreads();

  if (a.wave_r == 1) wave_sort_columns<T, 1>(keys, tc, ldk, tid);
  else if (a.wave_r == 2) wave_sort_columns<T, 2>(keys, tc, ldk, tid);
  else if (a.wave_r == 4) wave_sort_columns<T, 4>(keys, tc, ldk, tid);
  if (a.wave_r) __syncthreads();

  // longer columns: the network in LDS over every column of the tile at once
  const int half = npad >> 1, loghalf = a.lognp - 1;
  const int ces = half << a.logtc;
  for (int k = 2; k <= npad && !a.wave_r; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int e = tid; e < ces; e += ET) {
        const int col = e >> loghalf;
        const int p = e & (half - 1);
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        const int l = i | j;
        const bool asc = (i & k) == 0;
        T* kc = keys + (size_t)col * ldk;
        const T u = kc[i], w = kc[l];
        const bool sw = (u > w) == asc;
        kc[i] = sw ? w : u;
        kc[l] = sw ? u : w;
      }
      __syncthreads();
    }
  }

  if (!COVER) {
    const int evals = a.nq << a.logtc;
    for (int idx = tid; idx < evals; idx += ET) {
      const int col = idx & (tc - 1);
      const int k = idx >> a.logtc;
      const long long c = c0 + col;
      if (c >= a.cells) continue;
      const int m = ms[col];
      double r = NAN;
      if (m > 0 && !nanf[col]) r = lerp_quantile(keys + (size_t)col * ldk, m, a.q[k]);
      a.out[(long long)k * a.cells + c] = r;
    }
    if (a.n_eff)
      for (int col = tid; col < tc; col += ET)
        if (c0 + col < a.cells) a.n_eff[c0 + col] = ms[col];
  } else {
    const T* __restrict__ truth = static_cast<const T*>(a.truth);
    const int evals = a.K << a.logtc;
    for (int idx = tid; idx < evals; idx += ET) {
      const int col = idx & (tc - 1);
      const int k = idx >> a.logtc;
      const long long c = c0 + col;
      if (c >= a.cells) continue;
      const int m = ms[col];
      if (m < 1 || nanf[col]) continue;   // NaN bounds compare false
      const T* s = keys + (size_t)col * ldk;
      const double low = lerp_quantile(s, m, a.q_low[k]);
      const double upp = lerp_quantile(s, m, a.q_upp[k]);
      const double t = (double)truth[c];
      if (low < t && t <= upp) atomicAdd(&cnt[k * a.P + (int)(c % a.P)], 1);
    }
    for (int col = tid; col < tc; col += ET) {
      const long long c = c0 + col;
      if (c < a.cells && ms[col] >= 1) atomicAdd(&cnt[a.K * a.P + (int)(c % a.P)], 1);
    }
    __syncthreads();
    // integer adds: the totals do not depend on the order workgroups arrive in
    for (int i = tid; i < (a.K + 1) * a.P; i += ET) {
      const int v = cnt[i];
      if (v) atomicAdd(i < a.K * a.P ? &a.counts[i] : &a.cols[i - a.K * a.P], v);
    }
  }
}

// Mean and population variance per column, two passes (mean, then
// mean((x - mean)^2)), float64.  Block = cx columns x ry row groups: adjacent
// lanes on adjacent columns, every row group walks its rows, partials added in
// row-group order.
struct MomArgs {
  const void* x;
  int n;
  long long cells, ld;
  const uint8_t* valid;
  long long vcols;
  int rpv;
  int cx, logcx;
  double* mean;
  double* var;
};

template <typename T>
__global__ __launch_bounds__(ET) void ens_moments_kernel(MomArgs a) {
  __shared__ double part[ET];
  __shared__ int pcnt[ET];
  const int tid = threadIdx.x;
  const int cxi = tid & (a.cx - 1), ry = tid >> a.logcx, nry = ET >> a.logcx;
  const long long c = (long long)blockIdx.x * a.cx + cxi;
  const bool in = c < a.cells;
  const T* __restrict__ x = static_cast<const T*>(a.x);
  const long long vc = in && a.valid ? c / a.rpv : 0;

  double s = 0.0;
  int m = 0;
  if (in)
    for (int r = ry; r < a.n; r += nry) {
      if (a.valid && !a.valid[(long long)r * a.vcols + vc]) continue;
      s += (double)x[(long long)r * a.ld + c];
      ++m;
    }
  part[tid] = s;
  pcnt[tid] = m;
  __syncthreads();
  double tot = 0.0;
  int mt = 0;
  for (int g = 0; g < nry; ++g) {
    tot += part[(g << a.logcx) + cxi];
    mt += pcnt[(g << a.logcx) + cxi];
  }
  const double mean = tot / (double)mt;
  __syncthreads();
  double s2 = 0.0;
  if (in)
    for (int r = ry; r < a.n; r += nry) {
      if (a.valid && !a.valid[(long long)r * a.vcols + vc]) continue;
      const double d = (double)x[(long long)r * a.ld + c] - mean;
      s2 += d * d;
    }
  part[tid] = s2;
  __syncthreads();
  if (ry == 0 && in) {
    double t2 = 0.0;
    for (int g = 0; g < nry; ++g) t2 += part[(g << a.logcx) + cxi];
    a.mean[c] = mean;
    a.var[c] = t2 / (double)mt;
  }
}

// WSSE: out[s, e] = mean_m (pred[s,m,e] - obs[m,e])^2 / (A |obs[m,e]| + B)^2.
// One 1024-thread workgroup per realisation (n is ~100: 16 waves per
// workgroup keep enough loads in flight); thread (g, e) = (tid / eb, tid % eb)
// walks m = g, g + G, ..., so the workgroup reads the realisation's contiguous
// M*E block front to back.  Partials are added in row-group order.
constexpr int WT = 1024;

template <typename T>
__global__ __launch_bounds__(WT) void wsse_kernel(const T* __restrict__ pred,
                                                  const T* __restrict__ obs, long long M, int E,
                                                  double A, double B, double* __restrict__ out) {
  __shared__ double part[WT];
  const int tid = threadIdx.x;
  const int eb = E < WT ? E : WT;
  const int G = WT / eb;
  const int g = tid / eb, el = tid - g * eb;
  const T* ps = pred + (long long)blockIdx.x * M * E;
  for (int e0 = 0; e0 < E; e0 += eb) {
    const int e = e0 + el;
    double acc = 0.0;
    if (g < G && e < E)
      for (long long m = g; m < M; m += G) {
        const double o = (double)obs[m * E + e];
        const double d = (double)ps[m * E + e] - o;
        const double sd = A * fabs(o) + B;
        acc += (d * d) / (sd * sd);
      }
    part[tid] = acc;
    __syncthreads();
    if (g == 0 && e < E) {
      double tot = 0.0;
      for (int k = 0; k < G; ++k) tot += part[k * eb + el];
      out[(long long)blockIdx.x * E + e] = tot / (double)M;
    }
    __syncthreads();
  }
}

inline int ens_rc(hipError_t e) { return e == hipSuccess ? ERTD_OK : (int)e; }

inline int ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

// tile geometry for n rows of `sz`-byte keys; false when n is out of range
bool plan_tile(TileArgs& a, int n, long long cells, int sz) {
  if (n < 1 || n > MAX_N) return false;
  a.lognp = ilog2(n);
  if (n <= 64 * MAX_WAVE_R && a.lognp < 6) a.lognp = 6;   // a wave holds 64 keys per register
  a.npad = 1 << a.lognp;
  a.wave_r = n <= 64 * MAX_WAVE_R ? a.npad / 64 : 0;
  int tc = TILE_BYTES / sz / a.npad;
  tc = tc < 1 ? 1 : (tc > 256 ? 256 : tc);
  // enough workgroups for the chip before wide tiles; 128-byte row segments at least
  const int tc_min = 128 / sz;
  while (tc > tc_min && cells / tc < 512) tc >>= 1;
  a.tc = tc;
  a.logtc = ilog2(tc);
  a.ldk = tc > 1 ? a.npad + 1 : a.npad;
  return true;
}

size_t tile_lds(const TileArgs& a, int sz, int counters) {
  const size_t key_bytes = (((size_t)a.tc * a.ldk * sz) + 15) & ~(size_t)15;
  return key_bytes + (size_t)(2 * a.tc + counters) * sizeof(int);
}

template <typename T, bool COVER>
hipError_t launch_tile(const TileArgs& a, size_t lds, hipStream_t s) {
  static std::atomic<unsigned long long> done{0};
  if (lds > 64 * 1024)
    set_max_lds_once((const void*)ens_tile_kernel<T, COVER>, MAX_LDS, done);
  const long long blocks = (a.cells + a.tc - 1) / a.tc;
  ens_tile_kernel<T, COVER><<<(unsigned)blocks, ET, lds, s>>>(a);
  return hipGetLastError();
}

bool mask_ok(const unsigned char* valid, int rpv, long long cells) {
  return !valid || (rpv >= 1 && cells % rpv == 0);
}

}  // namespace
}  // namespace ertd

extern "C" {

int ertd_ens_percentile(const void* x, int dtype, int n, long long cells, long long ld,
                        const unsigned char* valid_rows, int rows_per_valid, const double* q,
                        int nq, double* out, int* n_eff, void* stream) {
  using namespace ertd;
  if (!x || !q || !out || nq < 1 || cells < 1 || ld < cells || cells > 0x7fffffffLL)
    return ERTD_EINVAL;
  if ((dtype != ERTD_F32 && dtype != ERTD_F64) || !mask_ok(valid_rows, rows_per_valid, cells))
    return ERTD_EINVAL;
  const int sz = dtype == ERTD_F32 ? 4 : 8;
  TileArgs a{};
  if (!plan_tile(a, n, cells, sz)) return ERTD_EINVAL;
  if ((long long)nq * a.tc > 0x7fffffffLL) return ERTD_EINVAL;
  a.x = x; a.n = n; a.cells = cells; a.ld = ld;
  a.valid = valid_rows; a.rpv = valid_rows ? rows_per_valid : 1; a.vcols = cells / a.rpv;
  a.q = q; a.nq = nq; a.out = out; a.n_eff = n_eff;
  const size_t lds = tile_lds(a, sz, 0);
  if (lds > (size_t)MAX_LDS) return ERTD_EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  return ens_rc(dtype == ERTD_F32 ? launch_tile<float, false>(a, lds, s)
                                  : launch_tile<double, false>(a, lds, s));
}

int ertd_ens_moments(const void* x, int dtype, int n, long long cells, long long ld,
                     const unsigned char* valid_rows, int rows_per_valid, double* mean,
                     double* var, void* stream) {
  using namespace ertd;
  if (!x || !mean || !var || n < 1 || cells < 1 || ld < cells || cells > 0x7fffffffLL)
    return ERTD_EINVAL;
  if ((dtype != ERTD_F32 && dtype != ERTD_F64) || !mask_ok(valid_rows, rows_per_valid, cells))
    return ERTD_EINVAL;
  MomArgs a{};
  a.x = x; a.n = n; a.cells = cells; a.ld = ld;
  a.valid = valid_rows; a.rpv = valid_rows ? rows_per_valid : 1; a.vcols = cells / a.rpv;
  // long columns: more row groups per column, 128-byte row segments still
  a.cx = n >= 1024 ? 16 : 64;
  a.logcx = ilog2(a.cx);
  a.mean = mean; a.var = var;
  const long long blocks = (cells + a.cx - 1) / a.cx;
  const hipStream_t s = (hipStream_t)stream;
  if (dtype == ERTD_F32) ens_moments_kernel<float><<<(unsigned)blocks, ET, 0, s>>>(a);
  else ens_moments_kernel<double><<<(unsigned)blocks, ET, 0, s>>>(a);
  return ens_rc(hipGetLastError());
}

int ertd_coverage(const void* ens, const void* truth, int dtype, int S, long long N, int P,
                  const unsigned char* valid_rows, const double* q_low, const double* q_upp, int K,
                  int* counts, int* cols, void* stream) {
  using namespace ertd;
  if (!ens || !truth || !q_low || !q_upp || !counts || !cols || N < 1 || P < 1 || K < 1)
    return ERTD_EINVAL;
  if (dtype != ERTD_F32 && dtype != ERTD_F64) return ERTD_EINVAL;
  if ((long long)(K + 1) * P > MAX_CNT || N * P > 0x7fffffffLL) return ERTD_EINVAL;
  const long long cells = N * P;
  const int sz = dtype == ERTD_F32 ? 4 : 8;
  TileArgs a{};
  if (!plan_tile(a, S, cells, sz)) return ERTD_EINVAL;
  a.x = ens; a.n = S; a.cells = cells; a.ld = cells;
  a.valid = valid_rows; a.rpv = valid_rows ? P : 1; a.vcols = cells / a.rpv;
  a.truth = truth; a.q_low = q_low; a.q_upp = q_upp; a.K = K; a.P = P;
  a.counts = counts; a.cols = cols;
  const size_t lds = tile_lds(a, sz, (K + 1) * P);
  if (lds > (size_t)MAX_LDS) return ERTD_EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)K * P * sizeof(int), s);
  if (e == hipSuccess) e = hipMemsetAsync(cols, 0, (size_t)P * sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  return ens_rc(dtype == ERTD_F32 ? launch_tile<float, true>(a, lds, s)
                                  : launch_tile<double, true>(a, lds, s));
}

int ertd_wsse(const void* pred, const void* obs, int dtype, int n, long long M, int E, double A,
              double B, double* out, void* stream) {
  using namespace ertd;
  if (!pred || !obs || !out || n < 1 || M < 1 || E < 1) return ERTD_EINVAL;
  if (dtype != ERTD_F32 && dtype != ERTD_F64) return ERTD_EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  if (dtype == ERTD_F32)
    wsse_kernel<float><<<(unsigned)n, WT, 0, s>>>((const float*)pred, (const float*)obs, M, E, A, B, out);
  else
    wsse_kernel<double><<<(unsigned)n, WT, 0, s>>>((const double*)pred, (const double*)obs, M, E, A, B,
                                                   out);
  return ens_rc(hipGetLastError());
}

}  // extern "C"
