// test_canaux_rythme.cc -- tsd_amd::filtre_rif_decim_canaux / filtre_rif_demi_bande_canaux / filtre_rif_ups_canaux /
// decimateur_canaux against C separate filtre_rif_decim / filtre_rif_demi_bande / filtre_rif_ups / decimateur objects, on
// host vectors and on resident (device) vectors: equal bits.  Built and run by tests/test_rate_bank_cpp_gpu.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include "dsp/dsp.hpp"
#include "dsp/filter.hpp"
#include "tsd_amd/extensions.hpp"

using namespace tsd;
using namespace tsd::filtrage;

static int nfail = 0;
#define CHECK(cond, ...)                                                     \
  do {                                                                       \
    if (!(cond)) {                                                           \
      nfail++;                                                               \
      printf("FAIL %s:%d  %s  -- ", __FILE__, __LINE__, #cond);              \
      printf(__VA_ARGS__);                                                   \
      printf("\n");                                                          \
    }                                                                        \
  } while (0)

template <typename T> static Vecteur<T> aleatoire(int n, unsigned graine)
{
  Vecteur<T> v(n);
  unsigned s = graine;
  auto u = [&s] {
    s = s * 1664525u + 1013904223u;
    return (float) ((s >> 8) & 0xffff) / 32768.0f - 1.0f;
  };
  for (int i = 0; i < n; i++) {
    if constexpr (std::is_same_v<T, float>) v(i) = u();
    else v(i) = T(u(), u());
  }
  return v;
}

// C channels of n samples per block, four blocks (one shorter than any rate here); `banc` against C objects made by `seul`
template <typename T, typename FB, typename FS> static void compare(const char *quoi, FB banc, FS seul, int C)
{
  const int tailles[4] = {4099, 1, 37, 5000};
  auto fb_h = banc(), fb_g = banc();
  std::vector<sptr<FiltreGen<T>>> seuls;
  for (int c = 0; c < C; c++) seuls.push_back(seul());
  for (int b = 0; b < 4; b++) {
    const int n = tailles[b];
    const Vecteur<T> x = aleatoire<T>(C * n, 17u + 31u * b);
    // the single objects first: they tell the output count of the block
    std::vector<Vecteur<T>> ys(C);
    for (int c = 0; c < C; c++) {
      Vecteur<T> xc(n);
      for (int i = 0; i < n; i++) xc(i) = x(c * n + i);
      seuls[c]->step(xc, ys[c]);
    }
    const int m = ys[0].rows();
    Vecteur<T> y_h;
    fb_h->step(x, y_h);
    CHECK(y_h.rows() == C * m, "%s: %d outputs for %d channels of %d", quoi, (int) y_h.rows(), C, m);
    if (y_h.rows() != C * m) return;
    for (int c = 0; c < C; c++)
      CHECK(ys[c].rows() == m && (m == 0 || std::memcmp(ys[c].data(), y_h.data() + (size_t) c * m, (size_t) m * sizeof(T)) == 0),
            "%s: channel %d of block %d differs from its own object", quoi, c, b);
    // resident: the input and a pre-sized output on device memory
    if (m == 0) {
      Vecteur<T> y0;
      T *dx = (T *) tsd_amd::alloue_gpu((size_t) C * n * sizeof(T));
      tsd_amd::copie_vers_gpu(dx, x.data(), (size_t) C * n * sizeof(T));
      fb_g->step(Vecteur<T>::map(dx, C * n), y0);
      tsd_amd::synchronise_gpu();
      tsd_amd::libere_gpu(dx);
      CHECK(y0.rows() == 0, "%s: %d outputs where none is due", quoi, (int) y0.rows());
      continue;
    }
    T *dx = (T *) tsd_amd::alloue_gpu((size_t) C * n * sizeof(T)), *dy = (T *) tsd_amd::alloue_gpu((size_t) C * m * sizeof(T));
    tsd_amd::copie_vers_gpu(dx, x.data(), (size_t) C * n * sizeof(T));
    {
      const Vecteur<T> xg = Vecteur<T>::map(dx, C * n);
      Vecteur<T> yg = Vecteur<T>::map(dy, C * m);
      fb_g->step(xg, yg);
      CHECK(yg.data() == dy && yg.est_sur_gpu(), "%s: a pre-sized mapped output must be written in place", quoi);
    }
    Vecteur<T> y_g(C * m);
    tsd_amd::copie_vers_hote(y_g.data(), dy, (size_t) C * m * sizeof(T));
    tsd_amd::libere_gpu(dx);
    tsd_amd::libere_gpu(dy);
    CHECK(std::memcmp(y_g.data(), y_h.data(), (size_t) C * m * sizeof(T)) == 0, "%s: resident and host banks differ, block %d", quoi, b);
  }
}

int main()
{
  const int C = 5;
  const Vecf h31 = design_rif_fen(31, "lp", 0.1f), h15 = design_rif_fen(15, "lp", 0.2f), h24 = design_rif_fen(24, "lp", 0.1f);
  compare<float>("filtre_rif_decim_canaux<float,float> R=4", [&] { return tsd_amd::filtre_rif_decim_canaux<float, float>(h31, 4, C); },
                 [&] { return filtre_rif_decim<float, float>(h31, 4); }, C);
  compare<cfloat>("filtre_rif_decim_canaux<float,cfloat> R=4", [&] { return tsd_amd::filtre_rif_decim_canaux<float, cfloat>(h31, 4, C); },
                  [&] { return filtre_rif_decim<float, cfloat>(h31, 4); }, C);
  compare<float>("filtre_rif_decim_canaux<float,float> R=5", [&] { return tsd_amd::filtre_rif_decim_canaux<float, float>(h31, 5, C); },
                 [&] { return filtre_rif_decim<float, float>(h31, 5); }, C);
  compare<float>("filtre_rif_demi_bande_canaux<float,float>", [&] { return tsd_amd::filtre_rif_demi_bande_canaux<float, float>(h15, C); },
                 [&] { return filtre_rif_demi_bande<float, float>(h15); }, C);
  compare<cfloat>("filtre_rif_demi_bande_canaux<float,cfloat>", [&] { return tsd_amd::filtre_rif_demi_bande_canaux<float, cfloat>(h15, C); },
                  [&] { return filtre_rif_demi_bande<float, cfloat>(h15); }, C);
  compare<float>("filtre_rif_ups_canaux<float,float> R=2", [&] { return tsd_amd::filtre_rif_ups_canaux<float, float>(h31, 2, C); },
                 [&] { return filtre_rif_ups<float, float>(h31, 2); }, C);
  compare<cfloat>("filtre_rif_ups_canaux<float,cfloat> R=3", [&] { return tsd_amd::filtre_rif_ups_canaux<float, cfloat>(h24, 3, C); },
                  [&] { return filtre_rif_ups<float, cfloat>(h24, 3); }, C);
  compare<float>("decimateur_canaux<float> R=7", [&] { return tsd_amd::decimateur_canaux<float>(7, C); }, [&] { return decimateur<float>(7); }, C);
  compare<cfloat>("decimateur_canaux<cfloat> R=3", [&] { return tsd_amd::decimateur_canaux<cfloat>(3, C); }, [&] { return decimateur<cfloat>(3); }, C);
  bool threw = false;
  try {
    auto f = tsd_amd::filtre_rif_decim_canaux<float, float>(h31, 4, C);
    Vecf x(C * 10 + 1), y;
    f->step(x, y);
  } catch (...) {
    threw = true;
  }
  CHECK(threw, "a vector that is not C blocks of the same length must be refused");
  threw = false;
  try {
    auto f = tsd_amd::filtre_rif_decim_canaux<float, float>(h31, 100, C);
  } catch (...) {
    threw = true;
  }
  CHECK(threw, "a rate the bank does not serve must be refused by the factory");
  if (nfail) {
    printf("%d failure(s)\n", nfail);
    return 1;
  }
  printf("test_canaux_rythme OK\n");
  return 0;
}
