// Host check of the feature-GEMM statistics kernel's tile plan (lc_kernels.h: ft_feature, ft_deal): for every instance
// launch_ss_feat can take, every feature of the active width is computed exactly once, nothing reads past the staged row,
// and the 8-wave deal loads no SIMD with more than its share.  Prints one line per failure and "ok N" at the end.
#include <cstdio>
#include <vector>

#include "lc_kernels.h"

using namespace lck;

static int fails = 0;
#define CHECK(c, ...)                  \
  do {                                 \
    if (!(c)) {                        \
      ++fails;                         \
      if (fails < 50) {                \
        std::printf("FAIL " __VA_ARGS__); \
        std::printf("\n");             \
      }                                \
    }                                  \
  } while (0)

static void check_features(int DP, int DC) {
  const int one = DP, tiles = ft_tiles(DC), nf = ft_features(DC);
  std::vector<int> prod(DC * DC, 0), lin(DC, 0);
  int count = 0;
  for (int f = 0; f < 16 * tiles; ++f) {
    const FtFeature x = ft_feature(DC, one, f);
    CHECK((x.u < DC || x.u == one) && (x.w < DC || x.w == one) && x.u >= 0 && x.w >= 0, "DP %d DC %d f %d: columns %d %d",
          DP, DC, f, x.u, x.w);
    if (x.kind == FT_PRODUCT) {
      CHECK(x.u < DC && x.w < DC && x.u <= x.w, "DP %d DC %d f %d: product %d %d", DP, DC, f, x.u, x.w);
      if (x.u < DC && x.w < DC) ++prod[x.u * DC + x.w];
    } else if (x.kind == FT_LINEAR) {
      CHECK(x.u < DC && x.w == one, "DP %d DC %d f %d: linear %d %d", DP, DC, f, x.u, x.w);
      if (x.u < DC) ++lin[x.u];
    } else if (x.kind == FT_COUNT) {
      CHECK(x.u == one && x.w == one && f == nf - 1, "DP %d DC %d f %d: count", DP, DC, f);
      ++count;
    } else {
      CHECK(x.kind == FT_SPARE && x.u == one && x.w == one && f >= nf, "DP %d DC %d f %d: spare", DP, DC, f);
    }
  }
  for (int i = 0; i < DC; ++i) {
    CHECK(lin[i] == 1, "DP %d DC %d: linear feature %d x %d", DP, DC, i, lin[i]);
    for (int j = 0; j < DC; ++j)
      CHECK(prod[i * DC + j] == (i <= j ? 1 : 0), "DP %d DC %d: product (%d, %d) x %d", DP, DC, i, j, prod[i * DC + j]);
  }
  CHECK(count == 1, "DP %d DC %d: N_k x %d", DP, DC, count);
  CHECK(tiles == (nf + 15) / 16 && 16 * tiles - nf < 16, "DP %d DC %d: tiles", DP, DC);
}

static void check_deal(int DP, int DC, int NQ) {
  const int tiles = ft_tiles(DC), nsl = ft_nslice(DP, DC, NQ), waves = ft_waves(DP), tpw = ft_tpw(DP, DC, NQ);
  CHECK(tpw <= ft_tpw_max(DP, NQ) && tpw * NQ <= 72, "DP %d DC %d NQ %d: %d tiles per wave", DP, DC, NQ, tpw);
  std::vector<int> seen(nsl * waves * tpw + 1, 0);
  int maxsimd = 0;
  for (int sl = 0; sl < nsl; ++sl) {
    int simd[4] = {0, 0, 0, 0};
    for (int w = 0; w < waves; ++w) {
      int t0 = -1, nt = -1;
      ft_deal(DP, DC, NQ, sl, w, &t0, &nt);
      CHECK(nt >= 0 && nt <= tpw && t0 >= 0, "DP %d DC %d NQ %d slice %d wave %d: t0 %d nt %d", DP, DC, NQ, sl, w, t0, nt);
      if (waves == 8) CHECK(nt == tpw || nt == tpw - 1, "DP %d DC %d NQ %d: wave of %d tiles (tpw %d)", DP, DC, NQ, nt, tpw);
      for (int t = t0; t < t0 + nt && t >= 0 && t < (int)seen.size(); ++t) ++seen[t];
      simd[w % 4] += nt;
    }
    for (int s = 0; s < 4; ++s) maxsimd = simd[s] > maxsimd ? simd[s] : maxsimd;
  }
  for (int t = 0; t < (int)seen.size(); ++t)
    CHECK(seen[t] == (t < tiles ? 1 : 0), "DP %d DC %d NQ %d: tile %d dealt %d times", DP, DC, NQ, t, seen[t]);
  if (waves == 8) {
    const int share = (tiles + 4 * nsl - 1) / (4 * nsl);
    CHECK(maxsimd == share, "DP %d DC %d NQ %d: busiest SIMD %d tiles, share %d", DP, DC, NQ, maxsimd, share);
    CHECK(ft_nt_min(DP, DC, NQ) >= tpw - 1, "DP %d DC %d NQ %d: nt_min", DP, DC, NQ);
  }
  std::printf("DP %3d DC %3d NQ %2d: %3d tiles, %2d blocks of %d waves, <= %d per wave, busiest SIMD %d\n", DP, DC, NQ, tiles,
              nsl, waves, tpw, maxsimd);
}

int main() {
  int cases = 0;
  for (int DP = 32; DP <= 128; DP += 16) {
    std::vector<int> widths = {DP, DP - 8};
    if (DP <= 48) widths.push_back(DP - 4), widths.push_back(DP - 12);
    for (int DC : widths) {
      check_features(DP, DC);
      for (int NQ : {2, 4, 5, 6, 7, 8, 16}) {
        if (NQ == 16 && DP != 128) continue;
        check_deal(DP, DC, NQ);
        ++cases;
      }
    }
  }
  CHECK(ft_tiles(64) == 135, "D = 64: %d tiles", ft_tiles(64));
  int t0 = 0, nt = 0, maxsimd = 0;
  for (int sl = 0; sl < ft_nslice(64, 64, 8); ++sl)
    for (int s = 0; s < 4; ++s) {
      int load = 0;
      for (int w = s; w < 8; w += 4) ft_deal(64, 64, 8, sl, w, &t0, &nt), load += nt;
      maxsimd = load > maxsimd ? load : maxsimd;
    }
  CHECK(maxsimd == 17, "D = 64, 8 quads: busiest SIMD %d tiles", maxsimd);
  if (fails) return 1;
  std::printf("ok %d\n", cases);
  return 0;
}
