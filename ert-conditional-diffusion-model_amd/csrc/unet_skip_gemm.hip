// 1x1 convolution (the ResBlock skip projections, SURVEY 8a') as a batched
// GEMM on v_mfma_f32_32x32x16_bf16 with three-way split operands:
//   out[b][co][p] = bias[co] + sum_ci W[co][ci] x[b][ci][p]      (x = cat(srcA, srcB))
//
// Persistent workgroups walk (MT co x NT px) output tiles of one sample each.
// K runs in chunks of KC input channels, double-buffered in LDS: the X chunk
// from the NCHW input (the two inputs of a skip concatenation read in place),
// the W chunk from the direct packing's [co tile 32][chunk][step pair 8]
// [lane 64][2] blocks (unet_pack.h, 4 KB per 32 co and 32 channels).
// Round 1-5 kernels for these shapes (the implicit GEMM conv_kernel<1, ...>
// and conv1x1_kernel) ran the U2 skips at 48-56 % of the fp32 peak; they still
// take the shapes this kernel does not.
//
// An fp32 number is exactly h + m + l with
// h = bf16(x), m = bf16(x - h), l = bf16((x - h) - m) (round to nearest even;
// both subtractions are exact).  Both operands are split while they are staged
// into LDS -- from the fp32 NCHW input and the direct weight packing -- and
// each 16-channel k-group is six MFMAs: W_l X_h, W_h X_l, W_m X_m, W_m X_h,
// W_h X_m into a "small" accumulator, then W_h X_h into the main one; the
// three dropped products are <= 2^-24 of the term.  The two accumulators are
// added once, in the epilogue: (main + small) + bias (+ residual).  (With one
// accumulator the five small products each cost the running sum one more fp32
// rounding per k-group and the K = 512 layers missed the accuracy gate.)  Not
// exact fp32 products, but fp32-class: rel-L2 0.4-0.8 x that of an fp32 conv
// against float64 (tests/test_gpu_skip_gemm_split.py).  Per output the order
// is fixed -- k-groups in ascending channel order -- and independent of the
// batch, the grid and the tile walk.  An inf input has planes (inf, nan, nan):
// outputs that fp32 gives as inf come out NaN (as do inputs within half a bf16
// ulp of FLT_MAX, whose h rounds to inf); finite outputs are not affected.
//   LDS per buffer and operand: three planes of [octet of 8 ch][row][8 bf16]
// (row = px for X, co for W): a lane's MFMA operand (8 consecutive k of one
// row) is one ds_read_b128, consecutive lanes read consecutive 16-B records
// (conflict-free), and each fragment is reused over the wave's blocks and the
// products it appears in (18 reads for 24 MFMAs).  8 waves in a 2 x 4 grid;
// a chunk's global loads are issued two chunks ahead into one of two register
// sets and split and stored one chunk ahead (one barrier per chunk).
#include <type_traits>

#include "unet.h"
#include "unet_pack.h"

namespace ertd {
namespace unet {

namespace {

constexpr int KC = 32;                      // input channels per block of the direct packing
using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) short;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

// two fp32 -> packed bf16, round to nearest even: v_cvt_pk_bf16_f32, the bits of
// bf16_bits (unet_conv_bf16.hip) for every finite input; inf stays inf and a
// NaN stays a NaN
__device__ __forceinline__ unsigned bf16_pk(float a, float b) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2));
}
// (a, b) -> the packed planes h = bf16(x), m = bf16(x - h), l = bf16((x - h) - m);
// both subtractions are exact in fp32, so h + m + l == x for finite x
__device__ __forceinline__ void split3(float a, float b, unsigned& h, unsigned& m, unsigned& l) {
  h = bf16_pk(a, b);
  a = a - __uint_as_float(h << 16);
  b = b - __uint_as_float(h & 0xffff0000u);
  m = bf16_pk(a, b);
  a = a - __uint_as_float(m << 16);
  b = b - __uint_as_float(m & 0xffff0000u);
  l = bf16_pk(a, b);
}

// MT co x NT px tile, KC input channels per chunk, NW waves in a 2 x NW/2 grid
template <int MT, int NT, int KC, int NW>
struct SsGeom {
  static constexpr int NTHR = NW * 64;
  static constexpr int WNT = NT / (NW / 2);             // pixels per wave
  static constexpr int TI = MT / 64, TJ = WNT / 32;     // 32x32 blocks per wave
  static constexpr int OCT = KC / 8;                    // 8-channel records per row and chunk
  static constexpr int XPL = OCT * NT * 16;             // bytes of one X plane: [octet][px][8 ch bf16]
  static constexpr int WPL = OCT * MT * 16;             // bytes of one W plane: [octet][co][8 ch bf16]
  static constexpr int BUF = 3 * (XPL + WPL);
  static constexpr size_t LDS = (size_t)2 * BUF;
  static constexpr int PXU = OCT * NT / 2 >= NTHR ? 2 : 1;   // pixels per X staging unit
  static constexpr int XUN = OCT * NT / PXU;            // X staging units: PXU px x 8 ch
  static constexpr int WUN = OCT * MT;                  // W staging units: 1 co x 8 ch
  static constexpr int XV = (XUN + NTHR - 1) / NTHR, WV = (WUN + NTHR - 1) / NTHR;
  static constexpr int PD = 2;                          // chunks of global loads in flight (2 or 4; 4 measured the same)
  static_assert(MT % 64 == 0 && WNT % 32 == 0 && (KC == 16 || KC == 32) && NW % 2 == 0, "tile");
};

template <int MT, int NT, int KC, int NW>
__global__ __launch_bounds__(NW * 64) void skip_gemm_split_kernel(ConvArgs a, int HW, int ntiles) {
  using G = SsGeom<MT, NT, KC, NW>;
  constexpr int TI = G::TI, TJ = G::TJ, OCT = G::OCT, NTHR = G::NTHR, PXU = G::PXU;
  extern __shared__ __attribute__((aligned(16))) char smem_s[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / (NW / 2), wn = wave % (NW / 2);
  const int h = lane >> 5, l32 = lane & 31;
  const int Cin = a.Cin, Ca = a.Ca, Cout = a.Cout;
  const int nchunk = Cin / KC, nchunk32 = Cin / 32;
  const int nN = HW / NT, nM = Cout / MT;
  // persistent: workgroup bid runs tiles bid, bid + grid, ... (tile = (sample,
  // pixel tile, co tile), co fastest: concurrent neighbours share the X tile),
  // as one chunk stream -- the next tile's first chunks are loaded during the
  // current tile's last ones, so the per-tile load latency is paid once
  const int nloc = (int)blockIdx.x < ntiles ? (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x : 0;
  const int gtot = nloc * nchunk;
  struct Tile { int b, m0, p0; };
  auto tile_of = [&](int il) {
    const int t = (int)blockIdx.x + il * (int)gridDim.x;
    const int mt = t % nM, r = t / nM;
    return Tile{r / nN, mt * MT, (r % nN) * NT};
  };

  // staging units of the thread.  X: unit u = PXU px x 8 ch, pixels PXU (u %
  // (NT / PXU)) .. of octet u / (NT / PXU), which is the same for a whole wave
  // (NT / PXU is a multiple of 64) -- channel and source pointer are scalar.
  // Where there are fewer units than threads, the threads past them load a
  // duplicate and store nothing: every wave issues the same loads in the same
  // order, which keeps the counted vmcnt waits below exact.  W: unit u = 8 ch
  // of one co: (co tile, octet, co & 31); channel octet og of the layer is
  // k-steps 8 (og & 1) .. + 7 of lane half (og >> 1) & 1 of 32-chunk og >> 2 in
  // the direct packing, so the unit's offset is a thread constant plus a
  // scalar per chunk.
  int xo[G::XV], xoff[G::XV], woff[G::WV];
#pragma unroll
  for (int i = 0; i < G::XV; ++i) {
    const int u = (tid + NTHR * i) % G::XUN;
    xo[i] = __builtin_amdgcn_readfirstlane(u / (NT / PXU));
    xoff[i] = PXU * (u % (NT / PXU));
  }
#pragma unroll
  for (int i = 0; i < G::WV; ++i) {
    const int u = (tid + NTHR * i) % G::WUN;
    const int col = u & 31, o = (u >> 5) % OCT, t = (u >> 5) / OCT;
    woff[i] = t * nchunk32 * 1024 + (o & 1) * 512 + (OCT == 4 ? (o >> 1) * 64 : 0) + col * 2;
  }
  // PD register sets: a chunk's loads are issued PD chunks ahead of its MFMAs
  // and are split and stored one chunk ahead (the MFMAs of one chunk are far
  // too short to cover a global load's latency)
  constexpr int PD = G::PD;
  f32x2 xr[PD][G::XV][8], wr[PD][G::WV][4];
  auto load = [&](int g, auto set) __attribute__((always_inline)) {
    constexpr int S = decltype(set)::value;
    const int il = g / nchunk, k = g - il * nchunk;
    const Tile tl = tile_of(il);
    const float* __restrict__ wp = a.wpk + (size_t)(tl.m0 / 32) * nchunk32 * 1024 +
                                   (OCT == 4 ? k * 1024 : (k >> 1) * 1024 + (k & 1) * 64);
    const float* __restrict__ pa = a.srcA + (size_t)tl.b * Ca * HW + tl.p0;
    const float* __restrict__ pb = a.srcB + ((size_t)tl.b * a.Cb - Ca) * HW + tl.p0;
#pragma unroll
    for (int i = 0; i < G::XV; ++i) {
      const int ci0 = (k * OCT + xo[i]) * 8;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int ci = ci0 + q;
        const float* src = (ci < Ca ? pa : pb) + (size_t)ci * HW;
        if constexpr (PXU == 2) xr[S][i][q] = *reinterpret_cast<const f32x2*>(src + xoff[i]);
        else xr[S][i][q].x = src[xoff[i]];
      }
    }
#pragma unroll
    for (int i = 0; i < G::WV; ++i) {
#pragma unroll
      for (int q = 0; q < 4; ++q) wr[S][i][q] = *reinterpret_cast<const f32x2*>(wp + woff[i] + q * 128);
    }
  };
  auto store = [&](int buf, auto set) __attribute__((always_inline)) {
    constexpr int S = decltype(set)::value;
    char* xs = smem_s + buf * G::BUF;
    char* ws = xs + 3 * G::XPL;
#pragma unroll
    for (int i = 0; i < G::XV; ++i) {
      const int u = tid + NTHR * i;
      if (G::XUN % NTHR && u >= G::XUN) break;
      const int pp = u % (NT / PXU), o = u / (NT / PXU);
      unsigned pl[PXU][3][4];               // [px][plane][channel pair]
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        split3(xr[S][i][2 * q].x, xr[S][i][2 * q + 1].x, pl[0][0][q], pl[0][1][q], pl[0][2][q]);
        if constexpr (PXU == 2)
          split3(xr[S][i][2 * q].y, xr[S][i][2 * q + 1].y, pl[1][0][q], pl[1][1][q], pl[1][2][q]);
      }
      char* d = xs + (o * NT + PXU * pp) * 16;
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int e = 0; e < PXU; ++e)
          *reinterpret_cast<u32x4*>(d + p * G::XPL + e * 16) = u32x4{pl[e][p][0], pl[e][p][1], pl[e][p][2], pl[e][p][3]};
    }
#pragma unroll
    for (int i = 0; i < G::WV; ++i) {
      const int u = tid + NTHR * i;
      if (G::WUN % NTHR && u >= G::WUN) break;
      const int col = u & 31, o = (u >> 5) % OCT, t = (u >> 5) / OCT;
      unsigned pl[3][4];
#pragma unroll
      for (int q = 0; q < 4; ++q) split3(wr[S][i][q].x, wr[S][i][q].y, pl[0][q], pl[1][q], pl[2][q]);
      char* d = ws + (o * MT + t * 32 + col) * 16;
#pragma unroll
      for (int p = 0; p < 3; ++p)
        *reinterpret_cast<u32x4*>(d + p * G::WPL) = u32x4{pl[p][0], pl[p][1], pl[p][2], pl[p][3]};
    }
  };

  // two accumulators per block: the h h products, and the five small cross
  // terms (<= 2^-8 of it), which would otherwise each cost the large sum one
  // more fp32 rounding per k-group; they meet once, in the epilogue
  f32x16 acc[TI][TJ], accs[TI][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j) acc[i][j] = accs[i][j] = f32x16{};
  // chunk g = set (mod PD): LDS buffer g & 1 and, PD chunks earlier, register set g % PD.
  // Loads and stores are unconditional -- past the end the last chunk is loaded
  // and staged again, into the buffer nobody reads any more -- so no path keeps
  // loads pending across the loop's back edge and the compiler's vmcnt waits
  // stay exact (a conditional load made every wave wait out the loads it had
  // just issued before its first MFMA).
  auto step = [&](int g, auto set) __attribute__((always_inline)) {
    constexpr int S = decltype(set)::value, buf = S & 1;
    const int il = g / nchunk, k = g - il * nchunk;
    load(g + PD < gtot ? g + PD : gtot - 1, set);
    const char* xb = smem_s + buf * G::BUF + (wn * G::WNT + l32) * 16;
    const char* wb = smem_s + buf * G::BUF + 3 * G::XPL + (wm * (MT / 2) + l32) * 16;
#pragma unroll
    for (int kg = 0; kg < KC / 16; ++kg) {
      const int o = 2 * kg + h;             // the lane's 8 channels of this 16-channel k-group
      bf16x8 av[3][TI], bv[3][TJ];
#pragma unroll
      for (int p = 0; p < 3; ++p) {
#pragma unroll
        for (int i = 0; i < TI; ++i)
          av[p][i] = *reinterpret_cast<const bf16x8*>(wb + p * G::WPL + (o * MT + i * 32) * 16);
#pragma unroll
        for (int j = 0; j < TJ; ++j)
          bv[p][j] = *reinterpret_cast<const bf16x8*>(xb + p * G::XPL + (o * NT + j * 32) * 16);
      }
      // W plane x X plane, small terms first: l h, h l, m m, m h, h m; then h h
      constexpr int PA[5] = {2, 0, 1, 1, 0}, PB[5] = {0, 2, 1, 0, 1};
#pragma unroll
      for (int t = 0; t < 5; ++t)
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < TJ; ++j)
            accs[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[PA[t]][i], bv[PB[t]][j], accs[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[0][i], bv[0][j], acc[i][j], 0, 0, 0);
    }
    store(buf ^ 1, std::integral_constant<int, (S + 1) % PD>{});
    if (k == nchunk - 1) {
      // epilogue: lane holds rows 8 (r / 4) + 4 h + (r % 4) of each 32 x 32 block,
      // column l32; a block row's bias and residual loads all issue before its
      // first store (out may alias nothing here, but the compiler cannot know:
      // interleaved, every load would wait out its own round trip)
      const Tile tl = tile_of(il);
      const size_t o0 = (size_t)tl.b * Cout * HW + tl.p0 + wn * G::WNT + l32;
      auto epilogue = [&](auto has_res) __attribute__((always_inline)) {
        constexpr bool RES = decltype(has_res)::value;
#pragma unroll
        for (int i = 0; i < TI; ++i) {
          const int co0 = tl.m0 + wm * (MT / 2) + i * 32 + 4 * h;
          float bi[16], rv[RES ? 16 : 1][TJ];
#pragma unroll
          for (int r = 0; r < 16; ++r) bi[r] = a.bias ? a.bias[co0 + 8 * (r >> 2) + (r & 3)] : 0.f;
          if constexpr (RES) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
              for (int j = 0; j < TJ; ++j)
                rv[r][j] = a.res[o0 + (size_t)(co0 + 8 * (r >> 2) + (r & 3)) * HW + j * 32];
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int co = co0 + 8 * (r >> 2) + (r & 3);
#pragma unroll
            for (int j = 0; j < TJ; ++j) {
              float v = (acc[i][j][r] + accs[i][j][r]) + bi[r];
              if constexpr (RES) v = v + rv[r][j];
              a.out[o0 + (size_t)co * HW + j * 32] = v;
            }
          }
        }
      };
      if (a.res) epilogue(std::true_type{});
      else epilogue(std::false_type{});
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) acc[i][j] = accs[i][j] = f32x16{};
    }
    __syncthreads();
  };
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;
  using S2 = std::integral_constant<int, 2>;
  using S3 = std::integral_constant<int, 3>;
  auto cl = [&](int c) { return c < gtot ? c : gtot - 1; };
  if (gtot > 0) {
    load(0, S0{});
    load(cl(1), S1{});
    if constexpr (PD == 4) {
      load(cl(2), S2{});
      load(cl(3), S3{});
    }
    store(0, S0{});
  }
  __syncthreads();
  int g = 0;
  for (; g + PD <= gtot; g += PD) {
    step(g, S0{});
    step(g + 1, S1{});
    if constexpr (PD == 4) {
      step(g + 2, S2{});
      step(g + 3, S3{});
    }
  }
  if (g < gtot) step(g, S0{});
  if (g + 1 < gtot) step(g + 1, S1{});
  if constexpr (PD == 4)
    if (g + 2 < gtot) step(g + 2, S2{});
}

template <int MT, int NT, int KC, int NW>
hipError_t launch_ss(const ConvArgs& a, int B, hipStream_t s, SkipGemmGeom* geom) {
  using G = SsGeom<MT, NT, KC, NW>;
  const int HW = a.Ho * a.Wo;
  static std::atomic<unsigned long long> attr{0};
  set_max_lds_once((const void*)skip_gemm_split_kernel<MT, NT, KC, NW>, (int)G::LDS, attr);
  // persistent grid: the workgroups that are resident at once
  static std::atomic<int> per_cu{0};
  int wpc = per_cu.load(std::memory_order_relaxed);
  if (wpc == 0) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&wpc, skip_gemm_split_kernel<MT, NT, KC, NW>, G::NTHR,
                                                     G::LDS) != hipSuccess || wpc < 1)
      wpc = 1;
    per_cu.store(wpc, std::memory_order_relaxed);
  }
  const int ntiles = HW / NT * (a.Cout / MT) * B;
  const int cap = wpc * device_cu_count();
  const int grid = ntiles < cap ? ntiles : cap;
  if (geom) {   // the query: this launch's geometry, nothing launched
    *geom = SkipGemmGeom{MT, NT, ntiles, grid};
    return hipSuccess;
  }
  skip_gemm_split_kernel<MT, NT, KC, NW><<<grid, G::NTHR, G::LDS, s>>>(a, HW, ntiles);
  return hipGetLastError();
}

// ERTD_SKIPGEMM (diagnostic builds): 0 keeps the round-5 kernels, 2 (the
// default) = the split-bf16 kernel at every shape it takes -- it measured
// faster at each of U2's 11 skips -- and the round-5 kernels
// elsewhere
int skip_gemm_env() {
  static const int v = [] {
    return ERTD_KNOB("SKIPGEMM", 2);
  }();
  return v;
}

}  // namespace

// ERTD_SG_TILE (diagnostic builds) forces the tile: 2 = 128 x 128, 3 = 64 x 256,
// 4 = 64 x 128, where it divides
static int sg_tile_env() {
  static const int v = [] {
    return ERTD_KNOB("SG_TILE", 0);
  }();
  return v;
}

// The split-bf16 kernel's tile: 128 x 128 where Cout is a multiple of 128, else
// 64 x 256 (the Cout = 64 skips at 64 x 64), 64 x 128 where 256 pixels do not
// divide HW.  Independent of B: a sample's bits do not depend on the batch --
// nor on the tile, round or workgroup of the persistent walk that computes it
// (the placement invariance stated at ertd_conv2d_route_info, include/ertdiff.h).
// false: the shape stays on the round-5 kernels.
constexpr int SS_KC = 32, SS_NW = 8;    // channels per chunk, waves per workgroup
static bool ss_tile(const ConvArgs& a, int& mt, int& nt) {
  if (skip_gemm_env() != 2 || a.Cout % 64) return false;
  const int HW = a.Ho * a.Wo;
  switch (sg_tile_env()) {
    case 2: mt = 128; nt = 128; break;
    case 3: mt = 64; nt = 256; break;
    case 4: mt = 64; nt = 128; break;
    default:
      mt = a.Cout % 128 ? 64 : 128;
      nt = mt == 128 ? 128 : (HW % 256 ? 128 : 256);
  }
  if (mt == 128 && a.Cout % 128) mt = 64;
  return HW % nt == 0;
}

template <int MT, int NT>
static hipError_t launch_ss_tile(const ConvArgs& a, int B, hipStream_t s, SkipGemmGeom* geom) {
#ifdef ERTD_DIAG
  // ERTD_SGS_KC = 16 / 32, ERTD_SGS_NW = 4 / 8: the schedule variants for A/B
  static const int kc = ERTD_KNOB("SGS_KC", SS_KC), nw = ERTD_KNOB("SGS_NW", SS_NW);
  if (kc == 16 && nw == 4) return launch_ss<MT, NT, 16, 4>(a, B, s, geom);
  if (kc == 16 && nw == 8) return launch_ss<MT, NT, 16, 8>(a, B, s, geom);
  if (kc == 32 && nw == 4) return launch_ss<MT, NT, 32, 4>(a, B, s, geom);
#endif
  return launch_ss<MT, NT, SS_KC, SS_NW>(a, B, s, geom);
}

bool skip_gemm_ok(const ConvArgs& a, int ks, int mode, int act, int B) {
  int mt, nt;
  return ks == 1 && mode == MODE_S1 && act == ACT_NONE && !a.ebias && !a.gnp &&
         a.Cin % KC == 0 && a.Ca % 4 == 0 && a.Cin == a.Ca + a.Cb && a.Ho == a.Hs && a.Wo == a.Ws &&
         a.wpk && ss_tile(a, mt, nt);
}

hipError_t launch_skip_gemm(const ConvArgs& a, int B, hipStream_t s, SkipGemmGeom* geom) {
  int mt, nt;
  if (!ss_tile(a, mt, nt)) return hipErrorInvalidValue;
  if (mt == 128) return launch_ss_tile<128, 128>(a, B, s, geom);
  if (nt == 256) return launch_ss_tile<64, 256>(a, B, s, geom);
  return launch_ss_tile<64, 128>(a, B, s, geom);
}

}  // namespace unet
}  // namespace ertd
