// test_synthetiseur.cc -- tsd_amd::synthetiseur_polyphase on host vectors and on resident (device) vectors against a plain
// double-precision loop of the definition
//     x[p] = sum_c exp(+2 pi i c p / M) sum_m u_c[m] f[p - m M],
// two steps per case, then canaliseur_polyphase -> filtre_rif_canaux -> synthetiseur_polyphase chained on resident vectors.
// Built and run by tests/test_synthesizer_cpp_gpu.py.
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

// M rows of F samples, row after row: uniform noise, plus a constant 1e3 in row 3
static Veccf lignes(int M, int F)
{
  Veccf v(M * F);
  unsigned s = 12345u;
  auto u = [&s] {
    s = s * 1664525u + 1013904223u;
    return (float) ((s >> 8) & 0xffff) / 32768.0f - 1.0f;
  };
  for (int c = 0; c < M; c++)
    for (int m = 0; m < F; m++) {
      const float re = u(), im = u();
      v(c * F + m) = cfloat(re + (c == 3 ? 1e3f : 0.f), im);
    }
  return v;
}

// the definition over the rows u[c * ld + m], m < F (frames before 0 are zeros): the F M samples of the stream
static std::vector<cd> definition(const std::vector<cd> &u, int ld, const Vecf &f, int M, int F)
{
  const int K = f.rows();
  const double PI = 3.14159265358979323846;
  std::vector<cd> x((size_t) M * F), w(M);
  for (int i = 0; i < M; i++) w[i] = cd(std::cos(2 * PI * i / M), std::sin(2 * PI * i / M));
  for (int p = 0; p < F * M; p++) {
    cd acc = 0;
    for (int c = 0; c < M; c++) {
      cd in = 0;
      for (int m = p / M; m >= 0 && p - m * M < K; m--) in += (double) f(p - m * M) * u[(size_t) c * ld + m];
      acc += in * w[(int) (((long long) c * p) % M)];
    }
    x[p] = acc;
  }
  return x;
}

static double ecart(const cfloat *x, const cd *ref, int n, double pk)
{
  double e = 0;
  for (int i = 0; i < n; i++) e = std::max(e, std::abs(cd(x[i].real(), x[i].imag()) - ref[i]));
  return e / pk;
}
static double crete(const std::vector<cd> &ref)
{
  double pk = 0;
  for (const cd &r : ref) pk = std::max(pk, std::abs(r));
  return pk;
}

static void compare(int M, int K, int F1, int F2)
{
  const int F = F1 + F2;
  const Vecf f = design_rif_fen(K, "lp", 0.5f / M);
  const Veccf u = lignes(M, F);
  std::vector<cd> ud((size_t) M * F);
  for (int i = 0; i < M * F; i++) ud[i] = cd(u(i).real(), u(i).imag());
  const std::vector<cd> ref = definition(ud, F, f, M, F);
  const double pk = crete(ref);
  auto f_h = tsd_amd::synthetiseur_polyphase(f, M), f_g = tsd_amd::synthetiseur_polyphase(f, M);
  int m0 = 0;
  for (int b = 0; b < 2; b++) {
    const int nf = b ? F2 : F1, n = nf * M;
    Veccf ub(n), x_h;
    for (int c = 0; c < M; c++)
      for (int m = 0; m < nf; m++) ub(c * nf + m) = u(c * F + m0 + m);
    f_h->step(ub, x_h);
    CHECK(x_h.rows() == n, "M=%d: %d outputs for %d blocks of %d", M, (int) x_h.rows(), M, nf);
    if (x_h.rows() != n) return;
    const double eh = ecart(x_h.data(), ref.data() + (size_t) m0 * M, n, pk);
    CHECK(eh <= 1e-5, "M=%d K=%d step %d (host): %.3g of the peak", M, K, b, eh);
    cfloat *du = (cfloat *) tsd_amd::alloue_gpu((size_t) n * sizeof(cfloat)), *dx = (cfloat *) tsd_amd::alloue_gpu((size_t) n * sizeof(cfloat));
    tsd_amd::copie_vers_gpu(du, ub.data(), (size_t) n * sizeof(cfloat));
    {
      const Veccf ug = Veccf::map(du, n);
      Veccf xg = Veccf::map(dx, n);
      f_g->step(ug, xg);
      CHECK(xg.data() == dx && xg.est_sur_gpu(), "M=%d: a pre-sized mapped output must be written in place", M);
    }
    Veccf x_g(n);
    tsd_amd::copie_vers_hote(x_g.data(), dx, (size_t) n * sizeof(cfloat));
    tsd_amd::libere_gpu(du);
    tsd_amd::libere_gpu(dx);
    CHECK(std::memcmp(x_g.data(), x_h.data(), (size_t) n * sizeof(cfloat)) == 0, "M=%d: resident and host runs differ, step %d", M, b);
    m0 += nf;
  }
}

// canaliseur_polyphase -> filtre_rif_canaux -> synthetiseur_polyphase on resident vectors; the synthesizer against the
// double-precision definition applied to the bank's output read back
static void chaine(int M, int K, int F)
{
  const Vecf h = design_rif_fen(K, "lp", 0.5f / M), h2 = design_rif_fen(15, "lp", 0.2f);
  const int n = F * M;
  Veccf x(n);
  const double PI = 3.14159265358979323846;
  for (int i = 0; i < n; i++) {
    const double a = 2 * PI * (3.3 / M) * i;
    x(i) = cfloat((float) (1e3 * std::cos(a)) + (float) ((i * 37) % 11) * 0.1f, (float) (1e3 * std::sin(a)) - (float) ((i * 53) % 7) * 0.1f);
  }
  auto can = tsd_amd::canaliseur_polyphase(h, M);
  auto banc = tsd_amd::filtre_rif_canaux<float, cfloat>(h2, M);
  auto syn = tsd_amd::synthetiseur_polyphase(h, M);
  cfloat *dx = (cfloat *) tsd_amd::alloue_gpu((size_t) n * sizeof(cfloat)), *dy = (cfloat *) tsd_amd::alloue_gpu((size_t) n * sizeof(cfloat)),
         *dz = (cfloat *) tsd_amd::alloue_gpu((size_t) n * sizeof(cfloat)), *dw = (cfloat *) tsd_amd::alloue_gpu((size_t) n * sizeof(cfloat));
  tsd_amd::copie_vers_gpu(dx, x.data(), (size_t) n * sizeof(cfloat));
  {
    const Veccf xg = Veccf::map(dx, n);
    Veccf yg = Veccf::map(dy, n), zg = Veccf::map(dz, n), wg = Veccf::map(dw, n);
    can->step(xg, yg);
    banc->step(yg, zg);
    syn->step(zg, wg);
    CHECK(wg.data() == dw && zg.data() == dz, "the chain must stay on the device");
  }
  Veccf z(n), w(n);
  tsd_amd::copie_vers_hote(z.data(), dz, (size_t) n * sizeof(cfloat));
  tsd_amd::copie_vers_hote(w.data(), dw, (size_t) n * sizeof(cfloat));
  tsd_amd::libere_gpu(dx);
  tsd_amd::libere_gpu(dy);
  tsd_amd::libere_gpu(dz);
  tsd_amd::libere_gpu(dw);
  std::vector<cd> zd((size_t) n);
  for (int i = 0; i < n; i++) zd[i] = cd(z(i).real(), z(i).imag());
  const std::vector<cd> ref = definition(zd, F, h, M, F);
  const double e = ecart(w.data(), ref.data(), n, crete(ref));
  CHECK(e <= 1e-5, "canaliseur_polyphase -> filtre_rif_canaux -> synthetiseur_polyphase, M=%d: %.3g of the peak", M, e);
}

int main()
{
  compare(8, 29, 21, 13);
  compare(256, 3 * 256 + 5, 5, 19);
  chaine(8, 29, 40);
  chaine(256, 2 * 256 + 1, 24);
  bool threw = false;
  try {
    auto f = tsd_amd::synthetiseur_polyphase(design_rif_fen(31, "lp", 0.05f), 8);
    Veccf x(8 * 10 + 1), y;
    f->step(x, y);
  } catch (...) {
    threw = true;
  }
  CHECK(threw, "a vector that is not nb_canaux blocks of one length must be refused");
  threw = false;
  try {
    auto f = tsd_amd::synthetiseur_polyphase(design_rif_fen(31, "lp", 0.05f), 8);
    Veccf x(8 * 10);
    f->step(x, x);
  } catch (...) {
    threw = true;
  }
  CHECK(threw, "x and y being the same vector must be refused");
  threw = false;
  try {
    auto f = tsd_amd::synthetiseur_polyphase(design_rif_fen(31, "lp", 0.05f), 12);
  } catch (...) {
    threw = true;
  }
  CHECK(threw, "a channel count the synthesizer does not serve must be refused by the factory");
  if (nfail) {
    printf("%d failure(s)\n", nfail);
    return 1;
  }
  printf("test_synthetiseur OK\n");
  return 0;
}
