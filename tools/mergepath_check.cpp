// Host check of csrc/mergepath.h, the index arithmetic of csrc/rowsort.hip.
// A development aid, run before the kernels first touch a GPU:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I ert-conditional-diffusion-model_amd/csrc tools/mergepath_check.cpp \
//       -o tools/mergepath_check && tools/mergepath_check
//
// 1. merge_path for every (la, lb, d) with la, lb <= 40 on tie-heavy keys
//    (5 distinct values, NaNs at the end), against the stable merge; the runs
//    are heap blocks of exactly la and lb keys, so a read past either traps.
// 2. The kernels' structure with small constants (tile 8, chunk 4 x 2 keys):
//    tile sort, merge passes by run_pair + chunk staging + per-thread walks,
//    for every M up to 150, against std::sort.
// 3. The chunked Wasserstein walk against the direct formula
//    sum |cdf_u - cdf_v| * diff(merged), term for term (bitwise).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "mergepath.h"

using namespace ertd;
typedef long long ll;

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (unsigned)(rng_state >> 32);
}

static bool less_d(double a, double b) { return mp::key_less(a, b); }
static bool same(double a, double b) { return (a != a && b != b) || a == b; }

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

// exact-size heap copy: the sanitizer traps any read outside
static std::unique_ptr<double[]> exact(const std::vector<double>& v) {
  std::unique_ptr<double[]> p(new double[v.size()]);
  if (!v.empty()) std::memcpy(p.get(), v.data(), v.size() * sizeof(double));
  return p;
}

static std::vector<double> keys(int n, int distinct, int nans) {
  std::vector<double> v(n);
  for (int i = 0; i < n; ++i) v[i] = distinct ? 0.25 * (rnd() % distinct) : (double)rnd() / 65536.0;
  for (int i = 0; i < nans && i < n; ++i) v[rnd() % n] = NAN;
  return v;
}

static void check_merge_path() {
  long cases = 0;
  for (int la = 0; la <= 40; ++la)
    for (int lb = 0; lb <= 40; ++lb)
      for (int variant = 0; variant < 3; ++variant) {
        std::vector<double> a = keys(la, variant == 2 ? 2 : 5, variant == 1 ? 2 : 0);
        std::vector<double> b = keys(lb, variant == 2 ? 2 : 5, variant == 1 ? 1 : 0);
        std::sort(a.begin(), a.end(), less_d);
        std::sort(b.begin(), b.end(), less_d);
        auto A = exact(a), B = exact(b);
        // stable merge, A first on ties: taken_a[d] keys of A among the first d
        std::vector<int> taken_a(la + lb + 1, 0);
        int i = 0, j = 0;
        for (int d = 0; d < la + lb; ++d) {
          const bool ta = mp::take_a(A.get(), (ll)la, (ll)i, B.get(), (ll)lb, (ll)j);
          CHECK(ta == (j >= lb || (i < la && !less_d(b[j], a[i]))));
          ta ? ++i : ++j;
          taken_a[d + 1] = i;
        }
        for (int d = 0; d <= la + lb; ++d, ++cases)
          CHECK(mp::merge_path(A.get(), (ll)la, B.get(), (ll)lb, (ll)d) == taken_a[d]);
      }
  std::printf("merge_path: %ld cases\n", cases);
}

// one workgroup of the merge pass / the integrate kernel: stage diagonals
// [d0, d1) into an exact-size block, return the A part's length
struct Staged {
  std::unique_ptr<double[]> sk;
  ll a0, b0;
  int na, nb;
};

static Staged stage(const double* A, ll la, const double* B, ll lb, ll d0, ll d1) {
  Staged s;
  s.a0 = mp::merge_path(A, la, B, lb, d0);
  s.b0 = d0 - s.a0;
  s.na = (int)(mp::merge_path(A, la, B, lb, d1) - s.a0);
  s.nb = (int)(d1 - d0) - s.na;
  CHECK(s.na >= 0 && s.nb >= 0 && s.a0 + s.na <= la && s.b0 + s.nb <= lb);
  s.sk.reset(new double[s.na + s.nb]);
  for (int i = 0; i < s.na + s.nb; ++i) s.sk[i] = i < s.na ? A[s.a0 + i] : B[s.b0 + (i - s.na)];
  return s;
}

static void check_sort(int tile, int threads, int items) {
  const int chunk = threads * items;
  long cases = 0;
  for (int M = 1; M <= 150; ++M)
    for (int variant = 0; variant < 3; ++variant, ++cases) {
      std::vector<double> x = keys(M, variant ? 5 : 0, variant == 2 ? 3 : 0);
      std::vector<double> want = x;
      std::sort(want.begin(), want.end(), less_d);
      std::vector<double> cur = x;
      const ll tiles = mp::ceil_div(M, tile);
      for (ll t = 0; t < tiles; ++t)
        std::sort(cur.begin() + t * tile, cur.begin() + std::min<ll>(M, (t + 1) * tile), less_d);
      const int passes = mp::merge_passes(tiles);
      ll L = tile;
      for (int p = 0; p < passes; ++p, L <<= 1) {
        auto src = exact(cur);
        std::vector<double> dst(M, -1.0);
        std::vector<char> written(M, 0);
        for (ll pos = 0; pos < M; pos += chunk) {
          const mp::RunPair r = mp::run_pair(M, L, pos);
          CHECK(r.la >= 1 && r.lb >= 0 && r.a0 + r.la <= M && r.b0 + r.lb <= M && r.d >= 0);
          CHECK(r.lb == 0 || r.b0 == r.a0 + r.la);
          const ll len = r.la + r.lb;
          const ll d1 = std::min<ll>(r.d + chunk, len);
          Staged s = stage(src.get() + r.a0, r.la, src.get() + r.b0, r.lb, r.d, d1);
          const int tot = s.na + s.nb;
          const double* sa = s.sk.get();
          const double* sb = sa + s.na;
          for (int tid = 0; tid < threads; ++tid) {
            const int dt = std::min(tid * items, tot);
            int ai = (int)mp::merge_path(sa, (ll)s.na, sb, (ll)s.nb, (ll)dt), bi = dt - ai;
            for (int k = 0; k < items && dt + k < tot; ++k) {
              const bool ta = mp::take_a(sa, (ll)s.na, (ll)ai, sb, (ll)s.nb, (ll)bi);
              CHECK(pos + dt + k < M && !written[pos + dt + k]);
              dst[pos + dt + k] = ta ? sa[ai++] : sb[bi++];
              written[pos + dt + k] = 1;
            }
          }
        }
        for (int i = 0; i < M; ++i) CHECK(written[i]);
        cur = dst;
      }
      for (int i = 0; i < M; ++i) CHECK(same(cur[i], want[i]));
    }
  std::printf("sort (tile %d, chunk %d x %d): %ld cases\n", tile, threads, items, cases);
}

static void check_w1(int threads, int items) {
  const int chunk = threads * items;
  long cases = 0;
  for (int Nu = 1; Nu <= 40; ++Nu)
    for (int Nv = 1; Nv <= 40; Nv += (Nu % 3) + 1)
      for (int variant = 0; variant < 2; ++variant, ++cases) {
        std::vector<double> u = keys(Nu, variant ? 5 : 0, 0), v = keys(Nv, variant ? 5 : 0, 0);
        std::sort(u.begin(), u.end());
        std::sort(v.begin(), v.end());
        const int N = Nu + Nv;
        // direct: the terms of scipy's _cdf_distance(p = 1), in order
        std::vector<double> all(u);
        all.insert(all.end(), v.begin(), v.end());
        std::sort(all.begin(), all.end());
        std::vector<double> want(N - 1);
        for (int k = 0; k + 1 < N; ++k) {
          const ll iu = std::upper_bound(u.begin(), u.end(), all[k]) - u.begin();
          const ll iv = std::upper_bound(v.begin(), v.end(), all[k]) - v.begin();
          want[k] = std::fabs((double)iu / (double)Nu - (double)iv / (double)Nv) * (all[k + 1] - all[k]);
        }
        auto U = exact(u), V = exact(v);
        std::vector<double> got(N - 1, -1.0);
        for (ll d0 = 0; d0 < N; d0 += chunk) {
          const ll d1 = std::min<ll>(d0 + chunk + 1, N);
          Staged s = stage(U.get(), Nu, V.get(), Nv, d0, d1);
          const int tot = s.na + s.nb;
          const double* sa = s.sk.get();
          const double* sb = sa + s.na;
          for (int tid = 0; tid < threads; ++tid) {
            const int dt = tid * items;
            if (dt >= tot) continue;
            int ai = (int)mp::merge_path(sa, (ll)s.na, sb, (ll)s.nb, (ll)dt), bi = dt - ai;
            bool ta = mp::take_a(sa, (ll)s.na, (ll)ai, sb, (ll)s.nb, (ll)bi);
            double c = ta ? sa[ai++] : sb[bi++];
            for (int k = 1; k <= items && dt + k < tot; ++k) {
              ta = mp::take_a(sa, (ll)s.na, (ll)ai, sb, (ll)s.nb, (ll)bi);
              const double next = ta ? sa[ai] : sb[bi];
              const double cu = (double)(s.a0 + ai) / (double)Nu, cv = (double)(s.b0 + bi) / (double)Nv;
              const ll term = d0 + dt + k - 1;
              CHECK(term < N - 1 && got[term] == -1.0);
              got[term] = std::fabs(cu - cv) * (next - c);
              ta ? ++ai : ++bi;
              c = next;
            }
          }
        }
        // a tied key's term is 0 in both; every other term carries the same bits
        for (int k = 0; k + 1 < N; ++k) CHECK(got[k] == want[k]);
      }
  std::printf("w1 walk (chunk %d x %d): %ld cases\n", threads, items, cases);
}

int main() {
  check_merge_path();
  check_sort(8, 4, 2);
  check_sort(16, 2, 4);
  check_sort(4, 1, 4);
  check_w1(4, 2);
  check_w1(1, 3);
  check_w1(8, 8);
  std::printf("ok\n");
  return 0;
}
