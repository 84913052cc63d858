// Batched sort of long contiguous rows and the Wasserstein-1 distance built
// on it (ertdiff/stats.py: sort_rows, wasserstein).
//
// Reference: ERT_Conditional_Diffusion.py
//   :860       wasserstein_distance(sim_data[idx].flatten(), observation.flatten())
//              for each of the best simulations
//   :898-899   the same for the ensemble mean and mode
// every call on 4693 x 14 = 65,702 values per side.
//
// Sort.  A row of M keys does not fit one workgroup's LDS (65,702 float64
// keys are 525 KB), so a row is sorted by many workgroups:
//   tile sort   one 1024-thread workgroup stages TILE keys of one row in LDS
//               (64 KiB of keys: 8192 float64 or 16384 float32; 72 KiB with
//               the bank padding, two workgroups per CU), pads the tail of a
//               short tile with NaN up to a power of two and runs the bitonic
//               network under np.sort's order (NaN last), three stages per
//               pass over LDS, then writes a sorted run;
//   merge pass  ceil(log2(runs)) ping-pong passes in global memory.  Every
//               256-thread workgroup produces CHUNK = 2048 consecutive keys of
//               one merged run: two lanes find the chunk's two input ranges by
//               a merge-path search (csrc/mergepath.h), the ranges (CHUNK keys
//               together) are staged in LDS, every thread finds its own 8
//               outputs by the same search in LDS and merges them serially.
//               An odd run at the end of a pass is the merge with an empty
//               partner: a copy.
// The run written by the tile sort alternates between `out` and the workspace
// so that the last pass lands in `out`.  Pass count and grids are functions of
// (n, M); no host synchronisation, no allocation, no atomics.
//
// Distance.  scipy.stats.wasserstein_distance without weights is
// _cdf_distance(p = 1):  sum_k |i_k / Nu - j_k / Nv| * (z[k+1] - z[k])  over the
// merged sorted sequence z of u and v, i_k and j_k the keys of u and v among
// z[0..k].  The integrate kernel walks that merge with the partition of the
// merge pass (chunks of 2048 merged keys plus the one that follows, 8 terms
// per thread), in float64, with the two real divisions scipy performs, so each
// term carries scipy's bits; a tied key contributes 0 in both.  Per-thread
// sums (chains of 8) are added in a fixed tree per workgroup, the workgroup
// partials per row by a last kernel: slices of consecutive partials per thread
// (at most 64 for the largest input), then the same tree.  No chain of
// sequential additions is longer than 64 terms and a term passes through at
// most 8 + 8 + 64 + 8 additions.  Sorting puts NaN last, so a row's result is
// NaN when the last sorted key of either side is.
#include "ertd_common.h"

#include <cmath>

#include "ertdiff.h"
#include "mergepath.h"

namespace ertd {
namespace {

using mp::key_less;
typedef long long ll;

constexpr int ST = 1024;                 // threads of the tile sort
constexpr int TILE_BYTES = 64 * 1024;    // keys of one tile in LDS
constexpr int MT = 256;                  // threads of a merge / integrate workgroup
constexpr int ITEMS = 8;                 // merged keys per thread
constexpr int CHUNK = MT * ITEMS;        // merged keys per workgroup
constexpr ll MAX_M = 1ll << 24;
constexpr ll MAX_BLOCKS = 1ll << 22;
constexpr size_t WS_ALIGN = 256;

// Key i of a tile lives at LDS slot i + i / 8.  The groups of the network start
// at stride bits s = 0, 3, 6, ...: at s = 0 adjacent lanes are 8 keys apart
// (8 lanes on one bank unpadded, 9 slots apart padded: none), at s = 3 every 8
// lanes jump 64 keys (4 lanes on one bank unpadded, 72 slots padded: none);
// from s = 6 on 32 adjacent lanes read 32 adjacent keys either way.
__host__ __device__ __forceinline__ int pad_index(int i) { return i + (i >> 3); }

// Stages of strides 2^(s+C-1) ... 2^s of merge step k over npad keys in LDS.
// Item p < npad >> C owns keys base + (r << s), r < 2^C, base = p with C zero
// bits inserted at bit s; every index is below npad.  The direction bit k lies
// above the group's stride bits, so it is one per item.
template <typename T, int C>
__device__ __forceinline__ void stage_group(T* keys, int npad, int k, int s, int tid) {
  constexpr int R = 1 << C;
  const int items = npad >> C;
  for (int p = tid; p < items; p += ST) {
    const int base = ((p >> s) << (s + C)) | (p & ((1 << s) - 1));
    const bool asc = (base & k) == 0;
    T v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = keys[pad_index(base + (r << s))];
#pragma unroll
    for (int b = R >> 1; b > 0; b >>= 1) {
#pragma unroll
      for (int r = 0; r < R; ++r)
        if ((r & b) == 0) {
          const T u = v[r], w = v[r | b];
          const bool sw = key_less(w, u) == asc;
          v[r] = sw ? w : u;
          v[r | b] = sw ? u : w;
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) keys[pad_index(base + (r << s))] = v[r];
  }
}

template <typename T>
__global__ __launch_bounds__(ST) void tile_sort_kernel(const T* __restrict__ x, ll ld, ll M,
                                                       int tile, ll tiles, T* __restrict__ dst) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* keys = reinterpret_cast<T*>(smem);
  const int tid = threadIdx.x;
  const ll row = blockIdx.x / tiles;
  const ll k0 = (blockIdx.x - row * tiles) * tile;
  const int cnt = (int)(M - k0 < tile ? M - k0 : tile);
  int npad = 2;
  while (npad < cnt) npad <<= 1;         // <= tile: a power of two
  const T* __restrict__ src = x + row * ld + k0;
  for (int i = tid; i < npad; i += ST) keys[pad_index(i)] = i < cnt ? src[i] : (T)NAN;
  __syncthreads();
  // the log2(k) stages of merge step k (strides k/2 ... 1) go three at a time
  // (the first group takes the remainder): a thread holds the 2^c keys whose
  // indices differ in the group's c stride bits, so one pass over LDS and one
  // barrier serve c stages -- 35 passes over a tile of 8192 instead of 91
  for (int k = 2, logk = 1; k <= npad; k <<= 1, ++logk) {
    for (int hi = logk - 1; hi >= 0;) {
      int c = (hi + 1) % 3;
      c = c ? c : 3;
      const int s = hi - c + 1;
      if (c == 3) stage_group<T, 3>(keys, npad, k, s, tid);
      else if (c == 2) stage_group<T, 2>(keys, npad, k, s, tid);
      else stage_group<T, 1>(keys, npad, k, s, tid);
      __syncthreads();
      hi = s - 1;
    }
  }
  T* __restrict__ o = dst + row * M + k0;
  for (int i = tid; i < cnt; i += ST) o[i] = keys[pad_index(i)];
}

// Stage the keys of diagonals [d0, d1) of merge(A, B) in LDS as K: the part
// from A at sk[0, na), the part from B at sk[na, na + nb); na + nb = d1 - d0.
// a0 / b0: the keys of A / B before diagonal d0.  sh: 2 words of LDS.
template <typename T, typename K>
__device__ __forceinline__ void stage_chunk(const T* __restrict__ A, ll la, const T* __restrict__ B,
                                            ll lb, ll d0, ll d1, K* sk, ll* sh, int tid, ll& a0,
                                            ll& b0, int& na, int& nb) {
  if (tid < 2) sh[tid] = mp::merge_path(A, la, B, lb, tid ? d1 : d0);
  __syncthreads();
  a0 = sh[0];
  b0 = d0 - a0;
  na = (int)(sh[1] - a0);
  nb = (int)(d1 - d0) - na;
  const int tot = na + nb;
  for (int i = tid; i < tot; i += MT) sk[i] = (K)(i < na ? A[a0 + i] : B[b0 + (i - na)]);
  __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(MT) void merge_pass_kernel(const T* __restrict__ src, T* __restrict__ dst,
                                                        ll M, ll L, ll chunks) {
  __shared__ T sk[CHUNK];
  __shared__ ll sh[2];
  const int tid = threadIdx.x;
  const ll row = blockIdx.x / chunks;
  const ll pos = (blockIdx.x - row * chunks) * CHUNK;
  const mp::RunPair r = mp::run_pair(M, L, pos);
  const T* __restrict__ A = src + row * M + r.a0;
  const T* __restrict__ B = src + row * M + r.b0;
  const ll len = r.la + r.lb;
  const ll d1 = r.d + CHUNK < len ? r.d + CHUNK : len;
  ll a0, b0;
  int na, nb;
  stage_chunk<T, T>(A, r.la, B, r.lb, r.d, d1, sk, sh, tid, a0, b0, na, nb);
  const int tot = na + nb;
  const T* sa = sk;
  const T* sb = sk + na;
  const int dt = tid * ITEMS < tot ? tid * ITEMS : tot;
  int ai = (int)mp::merge_path(sa, (ll)na, sb, (ll)nb, (ll)dt);
  int bi = dt - ai;
  T o[ITEMS];
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) {
    o[k] = (T)0;
    if (dt + k < tot) {
      const bool ta = mp::take_a(sa, (ll)na, (ll)ai, sb, (ll)nb, (ll)bi);
      o[k] = ta ? sa[ai] : sb[bi];
      ai += ta ? 1 : 0;
      bi += ta ? 0 : 1;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < ITEMS; ++k)
    if (dt + k < tot) sk[dt + k] = o[k];
  __syncthreads();
  T* __restrict__ out = dst + row * M + pos;
  for (int i = tid; i < tot; i += MT) out[i] = sk[i];
}

// fixed tree over the workgroup's MT values; the total is in part[0]
__device__ __forceinline__ void tree_sum(double* part, int tid) {
  for (int s = MT / 2; s > 0; s >>= 1) {
    __syncthreads();
    if (tid < s) part[tid] += part[tid + s];
  }
  __syncthreads();
}

// us: (n, Mu) sorted rows; vs: (Mv) sorted; partial: (n, nblk)
template <typename T>
__global__ __launch_bounds__(MT) void w1_integrate_kernel(const T* __restrict__ us, ll Mu,
                                                          const T* __restrict__ vs, ll Mv, ll nblk,
                                                          double* __restrict__ partial) {
  __shared__ double sk[CHUNK + 1];
  __shared__ double part[MT];
  __shared__ ll sh[2];
  const int tid = threadIdx.x;
  const ll row = blockIdx.x / nblk;
  const ll d0 = (blockIdx.x - row * nblk) * CHUNK;
  const ll N = Mu + Mv;
  const ll d1 = d0 + CHUNK + 1 < N ? d0 + CHUNK + 1 : N;   // one key past the chunk: the last `next`
  ll a0, b0;
  int na, nb;
  stage_chunk<T, double>(us + row * Mu, Mu, vs, Mv, d0, d1, sk, sh, tid, a0, b0, na, nb);
  const int tot = na + nb;
  const double* sa = sk;
  const double* sb = sk + na;
  const double nu = (double)Mu, nv = (double)Mv;
  double acc = 0.0;
  const int dt = tid * ITEMS;
  if (dt < tot) {
    int ai = (int)mp::merge_path(sa, (ll)na, sb, (ll)nb, (ll)dt);
    int bi = dt - ai;
    bool ta = mp::take_a(sa, (ll)na, (ll)ai, sb, (ll)nb, (ll)bi);
    double cur = ta ? sa[ai] : sb[bi];
    ai += ta ? 1 : 0;
    bi += ta ? 0 : 1;
#pragma unroll
    for (int k = 1; k <= ITEMS; ++k) {
      if (dt + k < tot) {
        ta = mp::take_a(sa, (ll)na, (ll)ai, sb, (ll)nb, (ll)bi);
        const double next = ta ? sa[ai] : sb[bi];
        const double cu = (double)(a0 + ai) / nu;      // keys of u consumed so far
        const double cv = (double)(b0 + bi) / nv;
        acc += fabs(cu - cv) * (next - cur);
        ai += ta ? 1 : 0;
        bi += ta ? 0 : 1;
        cur = next;
      }
    }
  }
  part[tid] = acc;
  tree_sum(part, tid);
  if (tid == 0) partial[blockIdx.x] = part[0];
}

template <typename T>
__global__ __launch_bounds__(MT) void w1_final_kernel(const double* __restrict__ partial, ll nblk,
                                                      const T* __restrict__ us, ll Mu,
                                                      const T* __restrict__ vs, ll Mv,
                                                      double* __restrict__ out) {
  __shared__ double part[MT];
  const int tid = threadIdx.x;
  const ll row = blockIdx.x;
  const double* __restrict__ p = partial + row * nblk;
  const ll per = (nblk + MT - 1) / MT;
  const ll i0 = tid * per;
  const ll i1 = i0 + per < nblk ? i0 + per : nblk;
  double acc = 0.0;
  for (ll i = i0; i < i1; ++i) acc += p[i];
  part[tid] = acc;
  tree_sum(part, tid);
  if (tid == 0) {
    const T ul = us[row * Mu + Mu - 1], vl = vs[Mv - 1];
    out[row] = (ul != ul || vl != vl) ? (double)NAN : part[0];
  }
}

inline int rs_rc(hipError_t e) { return e == hipSuccess ? ERTD_OK : (int)e; }
inline size_t align_up(size_t b) { return (b + WS_ALIGN - 1) & ~(WS_ALIGN - 1); }
inline int tile_keys(int dtype) { return TILE_BYTES / (dtype == ERTD_F32 ? 4 : 8); }

// the shape checks every entry point shares
bool shape_ok(int dtype, int n, ll M) {
  if (dtype != ERTD_F32 && dtype != ERTD_F64) return false;
  if (n < 1 || M < 1 || M > MAX_M) return false;
  // one workgroup per tile, per chunk of a row and per chunk of a merged pair;
  // a grid's threads (1024 per tile) are counted in 32 bits
  return (ll)n * mp::ceil_div(2 * M, CHUNK) <= MAX_BLOCKS;
}

size_t sort_ws_bytes(int dtype, int n, ll M) {
  const ll tiles = mp::ceil_div(M, tile_keys(dtype));
  return tiles > 1 ? align_up((size_t)n * (size_t)M * (dtype == ERTD_F32 ? 4 : 8)) : 0;
}

template <typename T>
hipError_t sort_rows_launch(const T* x, int n, ll M, ll ld, T* out, T* ws, hipStream_t s) {
  const int tile = TILE_BYTES / (int)sizeof(T);
  const ll tiles = mp::ceil_div(M, tile);
  const int passes = mp::merge_passes(tiles);
  T* cur = (passes & 1) ? ws : out;       // the last pass writes `out`
  T* other = (passes & 1) ? out : ws;
  ll npad = 2;
  while (npad < M && npad < tile) npad <<= 1;
  const size_t lds = (size_t)pad_index((int)npad) * sizeof(T);   // 72 KiB for a full tile
  static std::atomic<unsigned long long> done{0};
  if (lds > 64 * 1024)
    set_max_lds_once((const void*)tile_sort_kernel<T>, pad_index(tile) * (int)sizeof(T), done);
  tile_sort_kernel<T><<<(unsigned)(n * tiles), ST, lds, s>>>(x, ld, M, tile, tiles, cur);
  hipError_t e = hipGetLastError();
  const ll chunks = mp::ceil_div(M, CHUNK);
  ll L = tile;
  for (int p = 0; p < passes && e == hipSuccess; ++p, L <<= 1) {
    merge_pass_kernel<T><<<(unsigned)(n * chunks), MT, 0, s>>>(cur, other, M, L, chunks);
    e = hipGetLastError();
    T* t = cur;
    cur = other;
    other = t;
  }
  return e;
}

struct W1Plan {
  size_t us, sort_ws, vs, part, total;   // byte offsets, then the size
  ll nblk;
};

W1Plan w1_plan(int dtype, int n, ll Mu, ll Mv) {
  const size_t sz = dtype == ERTD_F32 ? 4 : 8;
  W1Plan p{};
  p.nblk = mp::ceil_div(Mu + Mv, CHUNK);
  const size_t su = sort_ws_bytes(dtype, n, Mu), sv = sort_ws_bytes(dtype, 1, Mv);
  p.us = 0;
  p.sort_ws = p.us + align_up((size_t)n * (size_t)Mu * sz);
  p.vs = p.sort_ws + (su > sv ? su : sv);   // the two sorts run one after the other
  p.part = p.vs + align_up((size_t)Mv * sz);
  p.total = p.part + align_up((size_t)n * (size_t)p.nblk * sizeof(double));
  return p;
}

template <typename T>
hipError_t w1_launch(const T* u, int n, ll Mu, ll ld, const T* v, ll Mv, double* out, char* ws,
                     const W1Plan& p, hipStream_t s) {
  T* us = reinterpret_cast<T*>(ws + p.us);
  T* sw = reinterpret_cast<T*>(ws + p.sort_ws);
  T* vs = reinterpret_cast<T*>(ws + p.vs);
  double* part = reinterpret_cast<double*>(ws + p.part);
  hipError_t e = sort_rows_launch<T>(u, n, Mu, ld, us, sw, s);
  if (e != hipSuccess) return e;
  e = sort_rows_launch<T>(v, 1, Mv, Mv, vs, sw, s);
  if (e != hipSuccess) return e;
  w1_integrate_kernel<T><<<(unsigned)(n * p.nblk), MT, 0, s>>>(us, Mu, vs, Mv, p.nblk, part);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  w1_final_kernel<T><<<(unsigned)n, MT, 0, s>>>(part, p.nblk, us, Mu, vs, Mv, out);
  return hipGetLastError();
}

}  // namespace
}  // namespace ertd

extern "C" {

int ertd_rows_sort_tile(int dtype) {
  using namespace ertd;
  return (dtype == ERTD_F32 || dtype == ERTD_F64) ? tile_keys(dtype) : 0;
}

size_t ertd_rows_sort_ws_bytes(int dtype, int n, long long M) {
  using namespace ertd;
  return shape_ok(dtype, n, M) ? sort_ws_bytes(dtype, n, M) : 0;
}

int ertd_rows_sort(const void* x, int dtype, int n, long long M, long long ld, void* out, void* ws,
                   size_t ws_bytes, void* stream) {
  using namespace ertd;
  if (!shape_ok(dtype, n, M) || ld < M || !x || !out) return ERTD_EINVAL;
  const size_t need = sort_ws_bytes(dtype, n, M);
  if (ws_bytes < need) return ERTD_ENOSPC;
  if (need && !ws) return ERTD_EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  return rs_rc(dtype == ERTD_F32
                   ? sort_rows_launch<float>((const float*)x, n, M, ld, (float*)out, (float*)ws, s)
                   : sort_rows_launch<double>((const double*)x, n, M, ld, (double*)out, (double*)ws, s));
}

size_t ertd_wasserstein_ws_bytes(int dtype, int n, long long Mu, long long Mv) {
  using namespace ertd;
  if (!shape_ok(dtype, n, Mu) || !shape_ok(dtype, n, Mv)) return 0;
  return w1_plan(dtype, n, Mu, Mv).total;
}

int ertd_wasserstein(const void* u, int dtype, int n, long long Mu, long long ld, const void* v,
                     long long Mv, double* out, void* ws, size_t ws_bytes, void* stream) {
  using namespace ertd;
  if (!shape_ok(dtype, n, Mu) || !shape_ok(dtype, n, Mv) || ld < Mu || !u || !v || !out)
    return ERTD_EINVAL;
  const W1Plan p = w1_plan(dtype, n, Mu, Mv);
  if (ws_bytes < p.total) return ERTD_ENOSPC;
  if (!ws) return ERTD_EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  return rs_rc(dtype == ERTD_F32
                   ? w1_launch<float>((const float*)u, n, Mu, ld, (const float*)v, Mv, out, (char*)ws, p, s)
                   : w1_launch<double>((const double*)u, n, Mu, ld, (const double*)v, Mv, out, (char*)ws,
                                       p, s));
}

}  // extern "C"
