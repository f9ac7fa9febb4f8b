// test_canaux_ols.cc -- tsd_amd::filtre_rif_canaux(h, nb_canaux, méthode) on the overlap-save bank, float and cfloat data,
// 3 channels of 5000 samples, 127 taps, two steps: every channel's stream against the oracle's FiltreRIF (oracle/tsd_oracle.c),
// within 1e-5 of the reference's peak.  Built and run by tests/test_ols_bank_cpp_gpu.py.
#include <cmath>
#include <cstdio>
#include <vector>
#include "dsp/dsp.hpp"
#include "dsp/filter.hpp"
#include "tsd_amd/extensions.hpp"
extern "C" {
#include "tsd_oracle.h"
}

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

static void oracle_step(const Vecf &h, std::vector<float> &fen, int *index, const float *x, float *y, int n)
{
  orc_fir_ff(h.data(), (int) h.rows(), fen.data(), index, x, y, n);
}
static void oracle_step(const Vecf &h, std::vector<cfloat> &fen, int *index, const cfloat *x, cfloat *y, int n)
{
  orc_fir_cf(h.data(), (int) h.rows(), (orc_cf *) fen.data(), index, (const orc_cf *) x, (orc_cf *) y, n);
}

template <typename T> static void compare(const char *quoi, tsd_amd::MethodeRIF méthode)
{
  const int C = 3, n = 5000, K = 127;
  const Vecf h = design_rif_fen(K, "lp", 0.2f);
  auto banc = tsd_amd::filtre_rif_canaux<float, T>(h, C, méthode);
  std::vector<std::vector<T>> fen(C, std::vector<T>(K, T(0)));
  std::vector<int> index(C, 0);
  for (int pas = 0; pas < 2; pas++) {
    const Vecteur<T> x = aleatoire<T>(C * n, 17u + 31u * pas);
    Vecteur<T> y;
    banc->step(x, y);
    CHECK(y.rows() == C * n, "%s: %d outputs for %d inputs", quoi, (int) y.rows(), C * n);
    for (int c = 0; c < C; c++) {
      std::vector<T> ref(n);
      oracle_step(h, fen[c], &index[c], x.data() + c * n, ref.data(), n);
      float e = 0, m = 0;
      for (int i = 0; i < n; i++) {
        e = std::max(e, std::abs(y(c * n + i) - ref[i]));
        m = std::max(m, std::abs(ref[i]));
      }
      CHECK(e <= 1e-5f * m, "%s: channel %d of step %d is %g of the peak from the oracle", quoi, c, pas, e / m);
    }
  }
}

int main()
{
  compare<float>("filtre_rif_canaux<float,float> RIF_OLS", tsd_amd::RIF_OLS);
  compare<cfloat>("filtre_rif_canaux<float,cfloat> RIF_OLS", tsd_amd::RIF_OLS);
  compare<float>("filtre_rif_canaux<float,float> RIF_AUTO", tsd_amd::RIF_AUTO);
  compare<cfloat>("filtre_rif_canaux<float,cfloat> RIF_AUTO", tsd_amd::RIF_AUTO);
  compare<cfloat>("filtre_rif_canaux<float,cfloat> RIF_DIRECTE", tsd_amd::RIF_DIRECTE);
  if (nfail) {
    printf("%d failure(s)\n", nfail);
    return 1;
  }
  printf("test_canaux_ols OK\n");
  return 0;
}
