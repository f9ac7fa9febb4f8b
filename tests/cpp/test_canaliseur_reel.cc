// test_canaliseur_reel.cc -- tsd_amd::canaliseur_polyphase_reel on host vectors and on resident (device) vectors against a plain
// double-precision loop of the definition, rows c = 0 .. M / 2 only,
//     y_c[m] = sum_k h[k] x[n_m - k] exp(-2 pi i c (n_m - k) / M),  n_m = m M + M - 1,  x real,
// two steps.  Built and run by tests/test_rchannelizer_cpp_gpu.py.
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

static Vecf signal(int n, int M)
{
  Vecf v(n);
  unsigned s = 12345u;
  auto u = [&s] {
    s = s * 1664525u + 1013904223u;
    return (float) ((s >> 8) & 0xffff) / 32768.0f - 1.0f;
  };
  const double PI = 3.14159265358979323846;
  for (int i = 0; i < n; i++) v(i) = (float) (u() + 1e3 * std::cos(2 * PI * (3.3 / M) * i));
  return v;
}

// the definition over the whole stream x (positions before 0 are zeros): out[c * F + m], c <= M / 2
static std::vector<cd> definition(const Vecf &x, const Vecf &h, int M)
{
  const int F = x.rows() / M, K = h.rows(), C = M / 2 + 1;
  const double PI = 3.14159265358979323846;
  std::vector<cd> y((size_t) C * F), w(M);
  for (int i = 0; i < M; i++) w[i] = cd(std::cos(2 * PI * i / M), -std::sin(2 * PI * i / M));
  for (int m = 0; m < F; m++) {
    const int nm = m * M + M - 1;
    for (int c = 0; c < C; c++) {
      cd acc = 0;
      for (int k = 0; k < K && k <= nm; k++) {
        const int pos = nm - k;
        acc += (double) h(k) * (double) x(pos) * w[(int) (((long long) c * pos) % M)];
      }
      y[(size_t) c * F + m] = acc;
    }
  }
  return y;
}

static double ecart(const cfloat *y, int ld, const std::vector<cd> &ref, int F, int C, int m0, int nf)
{
  double e = 0, pk = 0;
  for (int c = 0; c < C; c++)
    for (int m = 0; m < nf; m++) {
      const cd r = ref[(size_t) c * F + m0 + m];
      e = std::max(e, std::abs(cd(y[(size_t) c * ld + m].real(), y[(size_t) c * ld + m].imag()) - r));
    }
  for (const cd &r : ref) pk = std::max(pk, std::abs(r));
  return e / pk;
}

static void compare(int M, int K, int F1, int F2)
{
  const int F = F1 + F2, C = M / 2 + 1;
  const Vecf h = design_rif_fen(K, "lp", 0.5f / M);
  const Vecf x = signal(F * M, M);
  const std::vector<cd> ref = definition(x, h, M);
  auto f_h = tsd_amd::canaliseur_polyphase_reel(h, M), f_g = tsd_amd::canaliseur_polyphase_reel(h, M);
  int m0 = 0;
  for (int b = 0; b < 2; b++) {
    const int nf = b ? F2 : F1, n = nf * M, no = C * nf;
    Vecf xb(n);
    Veccf y_h;
    for (int i = 0; i < n; i++) xb(i) = x(m0 * M + i);
    f_h->step(xb, y_h);
    CHECK(y_h.rows() == no, "M=%d: %d outputs for %d samples", M, (int) y_h.rows(), n);
    if (y_h.rows() != no) return;
    const double eh = ecart(y_h.data(), nf, ref, F, C, m0, nf);
    CHECK(eh <= 1e-5, "M=%d K=%d step %d (host): %.3g of the peak", M, K, b, eh);
    for (int m = 0; m < nf; m++)
      CHECK(y_h((C - 1) * nf + m).imag() == 0.0f && y_h(m).imag() == 0.0f, "M=%d: rows 0 and M / 2 must be exactly real (frame %d)", M, m);
    float *dx = (float *) tsd_amd::alloue_gpu((size_t) n * sizeof(float));
    cfloat *dy = (cfloat *) tsd_amd::alloue_gpu((size_t) no * sizeof(cfloat));
    tsd_amd::copie_vers_gpu(dx, xb.data(), (size_t) n * sizeof(float));
    {
      const Vecf xg = Vecf::map(dx, n);
      Veccf yg = Veccf::map(dy, no);
      f_g->step(xg, yg);
      CHECK(yg.data() == dy && yg.est_sur_gpu(), "M=%d: a pre-sized mapped output must be written in place", M);
    }
    Veccf y_g(no);
    tsd_amd::copie_vers_hote(y_g.data(), dy, (size_t) no * sizeof(cfloat));
    tsd_amd::libere_gpu(dx);
    tsd_amd::libere_gpu(dy);
    CHECK(std::memcmp(y_g.data(), y_h.data(), (size_t) no * sizeof(cfloat)) == 0, "M=%d: resident and host runs differ, step %d", M, b);
    m0 += nf;
  }
}

int main()
{
  compare(32, 100, 21, 13);
  bool threw = false;
  try {
    auto f = tsd_amd::canaliseur_polyphase_reel(design_rif_fen(31, "lp", 0.05f), 32);
    Vecf x(32 * 10 + 1);
    Veccf y;
    f->step(x, y);
  } catch (...) {
    threw = true;
  }
  CHECK(threw, "a vector that is not a whole number of frames must be refused");
  threw = false;
  try {
    auto f = tsd_amd::canaliseur_polyphase_reel(design_rif_fen(31, "lp", 0.05f), 8);
  } catch (...) {
    threw = true;
  }
  CHECK(threw, "a frame length the real-input channelizer does not serve must be refused by the factory");
  if (nfail) {
    printf("%d failure(s)\n", nfail);
    return 1;
  }
  printf("test_canaliseur_reel OK\n");
  return 0;
}
