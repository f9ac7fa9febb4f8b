// test_canaliseur_surech.cc -- tsd_amd::canaliseur_polyphase(h, nb_canaux, surech), the oversampled bank, on host vectors and on
// resident (device) vectors against a plain double-precision loop of the definition
//     y_c[m] = sum_k h[k] x[n_m - k] exp(-2 pi i c (n_m - k) / M),  n_m = m D + D - 1,  D = M / surech,
// two steps per case, the first of an odd number of hops: the second starts from real history and a non-zero phase.
// Built and run by tests/test_channelizer_os_cpp_gpu.py.
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

// the definition over the whole stream x (positions before 0 are zeros): out[c * F + m], F = n / D
static std::vector<cd> definition(const Veccf &x, const Vecf &h, int M, int D)
{
  const int F = x.rows() / D, K = h.rows();
  const double PI = 3.14159265358979323846;
  std::vector<cd> y((size_t) M * F), w(M);
  for (int i = 0; i < M; i++) w[i] = cd(std::cos(2 * PI * i / M), -std::sin(2 * PI * i / M));
  for (int m = 0; m < F; m++) {
    const int nm = m * D + D - 1;
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

static void compare(int M, int OS, int K, int F1, int F2)
{
  const int F = F1 + F2, D = M / OS;
  const Vecf h = design_rif_fen(K, "lp", 0.5f / M);
  const Veccf x = signal(F * D, M);
  const std::vector<cd> ref = definition(x, h, M, D);
  auto f_h = tsd_amd::canaliseur_polyphase(h, M, OS), f_g = tsd_amd::canaliseur_polyphase(h, M, OS);
  int m0 = 0;
  for (int b = 0; b < 2; b++) {
    const int nf = b ? F2 : F1, n = nf * D, no = nf * M;
    Veccf xb(n), y_h;
    for (int i = 0; i < n; i++) xb(i) = x(m0 * D + i);
    f_h->step(xb, y_h);
    CHECK(y_h.rows() == no, "M=%d OS=%d: %d outputs for %d samples", M, OS, (int) y_h.rows(), n);
    if (y_h.rows() != no) return;
    const double eh = ecart(y_h.data(), nf, ref, F, M, m0, nf);
    CHECK(eh <= 1e-5, "M=%d OS=%d K=%d step %d (host): %.3g of the peak", M, OS, K, b, eh);
    cfloat *dx = (cfloat *) tsd_amd::alloue_gpu((size_t) n * sizeof(cfloat)), *dy = (cfloat *) tsd_amd::alloue_gpu((size_t) no * sizeof(cfloat));
    tsd_amd::copie_vers_gpu(dx, xb.data(), (size_t) n * sizeof(cfloat));
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
  compare(64, 2, 3 * 64 + 5, 7, 12);
  // surech = 1 is the two-argument factory
  {
    const int M = 64, n = 10 * M;
    const Vecf h = design_rif_fen(2 * M + 1, "lp", 0.5f / M);
    const Veccf x = signal(n, M);
    Veccf y1, y2;
    tsd_amd::canaliseur_polyphase(h, M)->step(x, y1);
    tsd_amd::canaliseur_polyphase(h, M, 1)->step(x, y2);
    CHECK(y1.rows() == n && y2.rows() == n && std::memcmp(y1.data(), y2.data(), (size_t) n * sizeof(cfloat)) == 0,
          "surech = 1 must give the bits of the two-argument factory");
  }
  bool threw = false;
  try {
    auto f = tsd_amd::canaliseur_polyphase(design_rif_fen(31, "lp", 0.05f), 8, 2);
    Veccf x(4 * 10 + 1), y;
    f->step(x, y);
  } catch (...) {
    threw = true;
  }
  CHECK(threw, "a vector that is not a whole number of hops must be refused");
  threw = false;
  try {
    auto f = tsd_amd::canaliseur_polyphase(design_rif_fen(31, "lp", 0.05f), 8, 3);
  } catch (...) {
    threw = true;
  }
  CHECK(threw, "an oversampling the channelizer does not serve must be refused by the factory");
  if (nfail) {
    printf("%d failure(s)\n", nfail);
    return 1;
  }
  printf("test_canaliseur_surech OK\n");
  return 0;
}
