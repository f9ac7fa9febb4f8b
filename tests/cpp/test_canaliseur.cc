// test_canaliseur.cc -- tsd_amd::canaliseur_polyphase on host vectors and on resident (device) vectors against a plain
// double-precision loop of the definition
//     y_c[m] = sum_k h[k] x[n_m - k] exp(-2 pi i c (n_m - k) / M),  n_m = m M + M - 1,
// two steps per case, then canaliseur_polyphase -> filtre_rif_canaux chained on resident vectors.
// Built and run by tests/test_channelizer_cpp_gpu.py.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>
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

using cd = std::complex<double>;

static Veccf signal(int n, int M)
{
  Veccf v(n);
  unsigned s = 12345u;
  auto u = [&s] {
    s = s * 1664525u + 1013904223u;
    return (float) ((s >> 8) & 0xffff) / 32768.0f - 1.0f;
  };
  const double PI = 3.14159265358979323846;
  for (int i = 0; i < n; i++) {
    const double a = 2 * PI * (3.3 / M) * i;
    v(i) = cfloat((float) (u() + 1e3 * std::cos(a)), (float) (u() + 1e3 * std::sin(a)));
  }
  return v;
}

// the definition over the whole stream x (positions before 0 are zeros): out[c * F + m]
static std::vector<cd> definition(const Veccf &x, const Vecf &h, int M)
{
  const int F = x.rows() / M, K = h.rows();
  const double PI = 3.14159265358979323846;
  std::vector<cd> y((size_t) M * F), w(M);
  for (int i = 0; i < M; i++) w[i] = cd(std::cos(2 * PI * i / M), -std::sin(2 * PI * i / M));
  for (int m = 0; m < F; m++) {
    const int nm = m * M + M - 1;
    for (int c = 0; c < M; c++) {
      cd acc = 0;
      for (int k = 0; k < K && k <= nm; k++) {
        const int pos = nm - k;
        acc += (double) h(k) * cd(x(pos).real(), x(pos).imag()) * w[(int) (((long long) c * pos) % M)];
      }
      y[(size_t) c * F + m] = acc;
    }
  }
  return y;
}

static double ecart(const cfloat *y, int ld, const std::vector<cd> &ref, int F, int M, int m0, int nf)
{
  double e = 0, pk = 0;
  for (int c = 0; c < M; c++)
    for (int m = 0; m < nf; m++) {
      const cd r = ref[(size_t) c * F + m0 + m];
      e = std::max(e, std::abs(cd(y[(size_t) c * ld + m].real(), y[(size_t) c * ld + m].imag()) - r));
    }
  for (const cd &r : ref) pk = std::max(pk, std::abs(r));
  return e / pk;
}

static void compare(int M, int K, int F1, int F2)
{
  const int F = F1 + F2;
  const Vecf h = design_rif_fen(K, "lp", 0.5f / M);
  const Veccf x = signal(F * M, M);
  const std::vector<cd> ref = definition(x, h, M);
  auto f_h = tsd_amd::canaliseur_polyphase(h, M), f_g = tsd_amd::canaliseur_polyphase(h, M);
  int m0 = 0;
  for (int b = 0; b < 2; b++) {
    const int nf = b ? F2 : F1, n = nf * M;
    Veccf xb(n), y_h;
    for (int i = 0; i < n; i++) xb(i) = x(m0 * M + i);
    f_h->step(xb, y_h);
    CHECK(y_h.rows() == n, "M=%d: %d outputs for %d samples", M, (int) y_h.rows(), n);
    if (y_h.rows() != n) return;
    const double eh = ecart(y_h.data(), nf, ref, F, M, m0, nf);
    CHECK(eh <= 1e-5, "M=%d K=%d step %d (host): %.3g of the peak", M, K, b, eh);
    cfloat *dx = (cfloat *) tsd_amd::alloue_gpu((size_t) n * sizeof(cfloat)), *dy = (cfloat *) tsd_amd::alloue_gpu((size_t) n * sizeof(cfloat));
    tsd_amd::copie_vers_gpu(dx, xb.data(), (size_t) n * sizeof(cfloat));
    {
      const Veccf xg = Veccf::map(dx, n);
      Veccf yg = Veccf::map(dy, n);
      f_g->step(xg, yg);
      CHECK(yg.data() == dy && yg.est_sur_gpu(), "M=%d: a pre-sized mapped output must be written in place", M);
    }
    Veccf y_g(n);
    tsd_amd::copie_vers_hote(y_g.data(), dy, (size_t) n * sizeof(cfloat));
    tsd_amd::libere_gpu(dx);
    tsd_amd::libere_gpu(dy);
    CHECK(std::memcmp(y_g.data(), y_h.data(), (size_t) n * sizeof(cfloat)) == 0, "M=%d: resident and host runs differ, step %d", M, b);
    m0 += nf;
  }
}

// canaliseur_polyphase -> filtre_rif_canaux on resident vectors, against the double-precision composition
static void chaine(int M, int K, int F)
{
  const Vecf h = design_rif_fen(K, "lp", 0.5f / M), h2 = design_rif_fen(15, "lp", 0.2f);
  const int n = F * M;
  const Veccf x = signal(n, M);
  const std::vector<cd> ref = definition(x, h, M);
  std::vector<cd> ref2((size_t) M * F);
  for (int c = 0; c < M; c++)
    for (int m = 0; m < F; m++) {
      cd acc = 0;
      for (int k = 0; k < h2.rows() && k <= m; k++) acc += (double) h2(k) * ref[(size_t) c * F + m - k];
      ref2[(size_t) c * F + m] = acc;
    }
  auto can = tsd_amd::canaliseur_polyphase(h, M);
  auto banc = tsd_amd::filtre_rif_canaux<float, cfloat>(h2, M);
  cfloat *dx = (cfloat *) tsd_amd::alloue_gpu((size_t) n * sizeof(cfloat)), *dy = (cfloat *) tsd_amd::alloue_gpu((size_t) n * sizeof(cfloat)),
         *dz = (cfloat *) tsd_amd::alloue_gpu((size_t) n * sizeof(cfloat));
  tsd_amd::copie_vers_gpu(dx, x.data(), (size_t) n * sizeof(cfloat));
  {
    const Veccf xg = Veccf::map(dx, n);
    Veccf yg = Veccf::map(dy, n), zg = Veccf::map(dz, n);
    can->step(xg, yg);
    banc->step(yg, zg);
    CHECK(zg.data() == dz, "the chain must stay on the device");
  }
  Veccf z(n);
  tsd_amd::copie_vers_hote(z.data(), dz, (size_t) n * sizeof(cfloat));
  tsd_amd::libere_gpu(dx);
  tsd_amd::libere_gpu(dy);
  tsd_amd::libere_gpu(dz);
  const double e = ecart(z.data(), F, ref2, F, M, 0, F);
  CHECK(e <= 1e-5, "canaliseur_polyphase -> filtre_rif_canaux, M=%d: %.3g of the peak", M, e);
}

int main()
{
  compare(8, 29, 21, 13);
  compare(256, 3 * 256 + 5, 5, 19);
  chaine(8, 29, 40);
  chaine(256, 2 * 256 + 1, 24);
  bool threw = false;
  try {
    auto f = tsd_amd::canaliseur_polyphase(design_rif_fen(31, "lp", 0.05f), 8);
    Veccf x(8 * 10 + 1), y;
    f->step(x, y);
  } catch (...) {
    threw = true;
  }
  CHECK(threw, "a vector that is not a whole number of frames must be refused");
  threw = false;
  try {
    auto f = tsd_amd::canaliseur_polyphase(design_rif_fen(31, "lp", 0.05f), 12);
  } catch (...) {
    threw = true;
  }
  CHECK(threw, "a channel count the channelizer does not serve must be refused by the factory");
  if (nfail) {
    printf("%d failure(s)\n", nfail);
    return 1;
  }
  printf("test_canaliseur OK\n");
  return 0;
}
