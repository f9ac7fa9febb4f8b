// test_synthetiseur_surech.cc -- tsd_amd::synthetiseur_polyphase(h, nb_canaux, surech), the oversampled synthesis bank, on host
// vectors and on resident (device) vectors against a plain double-precision loop of the definition
//     x[p] = sum_c exp(+2 pi i c p / M) sum_m u_c[m] f[p - m D],  D = M / surech,  p counted over the whole stream,
// two steps per case, the first of an odd number of frames: the second starts from real history and a non-zero phase.
// Built and run by tests/test_synthesizer_os_cpp_gpu.py.
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

// rows[c * F + m]: noise plus a constant 1e3 in row 3
static std::vector<cfloat> rows(int M, int F)
{
  std::vector<cfloat> v((size_t) M * F);
  unsigned s = 12345u;
  auto u = [&s] {
    s = s * 1664525u + 1013904223u;
    return (float) ((s >> 8) & 0xffff) / 32768.0f - 1.0f;
  };
  for (int c = 0; c < M; c++)
    for (int m = 0; m < F; m++) {
      const float re = u(), im = u();
      v[(size_t) c * F + m] = cfloat(re + (c == 3 ? 1e3f : 0.f), im);
    }
  return v;
}

// the definition over the whole run (frames before 0 are zeros): F D samples
static std::vector<cd> definition(const std::vector<cfloat> &u, const Vecf &f, int M, int D, int F)
{
  const int K = f.rows();
  const double PI = 3.14159265358979323846;
  std::vector<cd> x((size_t) F * D), w(M);
  for (int i = 0; i < M; i++) w[i] = cd(std::cos(2 * PI * i / M), std::sin(2 * PI * i / M));
  for (int p = 0; p < F * D; p++) {
    cd acc = 0;
    for (int c = 0; c < M; c++) {
      cd in = 0;
      for (int m = 0; m < F && m * D <= p; m++) {
        const int k = p - m * D;
        if (k < K) in += (double) f(k) * cd(u[(size_t) c * F + m].real(), u[(size_t) c * F + m].imag());
      }
      acc += in * w[(int) (((long long) c * p) % M)];
    }
    x[p] = acc;
  }
  return x;
}

static void compare(int M, int OS, int K, int F1, int F2)
{
  const int F = F1 + F2, D = M / OS;
  const Vecf h = design_rif_fen(K, "lp", 0.5f / M);
  const std::vector<cfloat> u = rows(M, F);
  const std::vector<cd> ref = definition(u, h, M, D, F);
  double pk = 0;
  for (const cd &r : ref) pk = std::max(pk, std::abs(r));
  auto f_h = tsd_amd::synthetiseur_polyphase(h, M, OS), f_g = tsd_amd::synthetiseur_polyphase(h, M, OS);
  int m0 = 0;
  for (int b = 0; b < 2; b++) {
    const int nf = b ? F2 : F1, n = nf * M, no = nf * D;
    Veccf ub(n), y_h;
    for (int c = 0; c < M; c++)
      for (int m = 0; m < nf; m++) ub(c * nf + m) = u[(size_t) c * F + m0 + m];
    f_h->step(ub, y_h);
    CHECK(y_h.rows() == no, "M=%d OS=%d: %d outputs for %d frames", M, OS, (int) y_h.rows(), nf);
    if (y_h.rows() != no) return;
    double e = 0;
    for (int i = 0; i < no; i++) e = std::max(e, std::abs(cd(y_h(i).real(), y_h(i).imag()) - ref[(size_t) m0 * D + i]));
    CHECK(e / pk <= 1e-5, "M=%d OS=%d K=%d step %d (host): %.3g of the peak", M, OS, K, b, e / pk);
    cfloat *dx = (cfloat *) tsd_amd::alloue_gpu((size_t) n * sizeof(cfloat)), *dy = (cfloat *) tsd_amd::alloue_gpu((size_t) no * sizeof(cfloat));
    tsd_amd::copie_vers_gpu(dx, ub.data(), (size_t) n * sizeof(cfloat));
    {
      const Veccf xg = Veccf::map(dx, n);
      Veccf yg = Veccf::map(dy, no);
      f_g->step(xg, yg);
      CHECK(yg.data() == dy && yg.est_sur_gpu(), "M=%d OS=%d: a pre-sized mapped output must be written in place", M, OS);
    }
    Veccf y_g(no);
    tsd_amd::copie_vers_hote(y_g.data(), dy, (size_t) no * sizeof(cfloat));
    tsd_amd::libere_gpu(dx);
    tsd_amd::libere_gpu(dy);
    CHECK(std::memcmp(y_g.data(), y_h.data(), (size_t) no * sizeof(cfloat)) == 0, "M=%d OS=%d: resident and host runs differ, step %d", M, OS, b);
    m0 += nf;
  }
}

int main()
{
  compare(16, 2, 3 * 16 + 5, 7, 12);
  compare(64, 4, 5 * 16 + 3, 7, 10);
  // surech = 1 is the two-argument factory
  {
    const int M = 64, F = 10, n = F * M;
    const Vecf h = design_rif_fen(2 * M + 1, "lp", 0.5f / M);
    const std::vector<cfloat> u = rows(M, F);
    Veccf x(n), y1, y2;
    for (int i = 0; i < n; i++) x(i) = u[i];
    tsd_amd::synthetiseur_polyphase(h, M)->step(x, y1);
    tsd_amd::synthetiseur_polyphase(h, M, 1)->step(x, y2);
    CHECK(y1.rows() == n && y2.rows() == n && std::memcmp(y1.data(), y2.data(), (size_t) n * sizeof(cfloat)) == 0,
          "surech = 1 must give the bits of the two-argument factory");
  }
  bool threw = false;
  try {
    auto f = tsd_amd::synthetiseur_polyphase(design_rif_fen(31, "lp", 0.05f), 8, 2);
    Veccf x(8 * 10 + 1), y;
    f->step(x, y);
  } catch (...) {
    threw = true;
  }
  CHECK(threw, "a vector that is not nb_canaux blocks of one length must be refused");
  threw = false;
  try {
    auto f = tsd_amd::synthetiseur_polyphase(design_rif_fen(31, "lp", 0.05f), 8, 3);
  } catch (...) {
    threw = true;
  }
  CHECK(threw, "an oversampling the synthesizer does not serve must be refused by the factory");
  if (nfail) {
    printf("%d failure(s)\n", nfail);
    return 1;
  }
  printf("test_synthetiseur_surech OK\n");
  return 0;
}
