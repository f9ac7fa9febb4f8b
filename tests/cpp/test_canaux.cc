// test_canaux.cc -- tsd_amd::filtre_rif_canaux / filtre_sois_canaux against C separate filtre_rif / filtre_sois objects, on
// host vectors and on resident (device) vectors.  Built and run by tests/test_bank_cpp_gpu.py.
#include <cmath>
#include <cstdio>
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

// max |a - b| / max |b|
template <typename T> static float ecart_rel(const Vecteur<T> &a, const Vecteur<T> &b)
{
  float e = 0, m = 0;
  for (int i = 0; i < b.rows(); i++) {
    e = std::max(e, std::abs(a(i) - b(i)));
    m = std::max(m, std::abs(b(i)));
  }
  return m > 0 ? e / m : e;
}

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

// C channels of n samples per block, three blocks; `banc` against C objects made by `seul`, on host and on resident vectors
template <typename T, typename FB, typename FS> static void compare(const char *quoi, FB banc, FS seul, int C, float tol)
{
  const int tailles[3] = {4096, 37, 5000};
  auto fb_h = banc(), fb_g = banc();
  std::vector<sptr<FiltreGen<T>>> seuls;
  for (int c = 0; c < C; c++) seuls.push_back(seul());
  for (int b = 0; b < 3; b++) {
    const int n = tailles[b];
    const Vecteur<T> x = aleatoire<T>(C * n, 17u + 31u * b);
    Vecteur<T> y_h;
    fb_h->step(x, y_h);
    CHECK(y_h.rows() == C * n, "%s: %d outputs for %d inputs", quoi, (int) y_h.rows(), C * n);
    // resident: the input and a pre-sized output on device memory
    T *dx = (T *) tsd_amd::alloue_gpu((size_t) C * n * sizeof(T)), *dy = (T *) tsd_amd::alloue_gpu((size_t) C * n * sizeof(T));
    tsd_amd::copie_vers_gpu(dx, x.data(), (size_t) C * n * sizeof(T));
    {
      const Vecteur<T> xg = Vecteur<T>::map(dx, C * n);
      Vecteur<T> yg = Vecteur<T>::map(dy, C * n);
      fb_g->step(xg, yg);
      CHECK(yg.data() == dy && yg.est_sur_gpu(), "%s: a pre-sized mapped output must be written in place", quoi);
    }
    Vecteur<T> y_g(C * n);
    tsd_amd::copie_vers_hote(y_g.data(), dy, (size_t) C * n * sizeof(T));
    tsd_amd::libere_gpu(dx);
    tsd_amd::libere_gpu(dy);
    CHECK(ecart_rel(y_g, y_h) == 0.f, "%s: resident and host banks differ (%g), block %d", quoi, ecart_rel(y_g, y_h), b);
    for (int c = 0; c < C; c++) {
      Vecteur<T> xc(n), yc;
      for (int i = 0; i < n; i++) xc(i) = x(c * n + i);
      seuls[c]->step(xc, yc);
      Vecteur<T> bc(n);
      for (int i = 0; i < n; i++) bc(i) = y_h(c * n + i);
      const float e = ecart_rel(bc, yc);
      CHECK(e <= tol, "%s: channel %d of block %d is %g from its own object", quoi, c, b, e);
    }
  }
}

int main()
{
  const int C = 5;
  const Vecf h = design_rif_fen(31, "lp", 0.2f);
  const Veccf hc = aleatoire<cfloat>(127, 5u);
  compare<float>("filtre_rif_canaux<float,float>", [&] { return tsd_amd::filtre_rif_canaux<float, float>(h, C); },
                 [&] { return filtre_rif<float, float>(h); }, C, 2e-6f);
  compare<cfloat>("filtre_rif_canaux<float,cfloat>", [&] { return tsd_amd::filtre_rif_canaux<float, cfloat>(h, C); },
                  [&] { return filtre_rif<float, cfloat>(h); }, C, 2e-6f);
  compare<cfloat>("filtre_rif_canaux<cfloat,cfloat>", [&] { return tsd_amd::filtre_rif_canaux<cfloat, cfloat>(hc, C); },
                  [&] { return filtre_rif<cfloat, cfloat>(hc); }, C, 2e-6f);
  const FRat<cfloat> H6 = design_riia(6, "lp", "butt", 0.2f), H5 = design_riia(5, "lp", "butt", 0.1f);
  compare<float>("filtre_sois_canaux<float> DF2", [&] { return tsd_amd::filtre_sois_canaux<float>(H6, C); },
                 [&] { return filtre_sois<float>(H6); }, C, 1e-5f);
  compare<float>("filtre_sois_canaux<float> odd order DF1", [&] { return tsd_amd::filtre_sois_canaux<float>(H5, C, FormeDirecte1); },
                 [&] { return filtre_sois<float>(H5, FormeDirecte1); }, C, 1e-5f);
  compare<cfloat>("filtre_sois_canaux<cfloat>", [&] { return tsd_amd::filtre_sois_canaux<cfloat>(H6, C); },
                  [&] { return filtre_sois<cfloat>(H6); }, C, 1e-5f);
  bool threw = false;
  try {
    auto f = tsd_amd::filtre_rif_canaux<float, float>(h, C);
    Vecf x(C * 10 + 1), y;
    f->step(x, y);
  } catch (...) {
    threw = true;
  }
  CHECK(threw, "a vector that is not C blocks of the same length must be refused");
  if (nfail) {
    printf("%d failure(s)\n", nfail);
    return 1;
  }
  printf("test_canaux OK\n");
  return 0;
}
