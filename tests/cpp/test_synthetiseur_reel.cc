// test_synthetiseur_reel.cc -- tsd_amd::synthetiseur_polyphase_reel on host vectors and on resident (device) vectors against a plain
// double-precision loop of the definition, with N = M / 2 and rows c = 0 .. N,
//     x[p] = sum_m f[p - m M] ( Re u_0[m] + (-1)^p Re u_N[m] + 2 sum_{0<c<N} Re( u_c[m] exp(+2 pi i c p / M) ) ),
// two steps, and against the bits of the C ABI (tsdgpu_synthesizer_create_real).  Built and run by
// tests/test_rsynthesizer_cpp_gpu.py.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>
#include "dsp/dsp.hpp"
#include "dsp/filter.hpp"
#include "tsd_amd/extensions.hpp"
#include "tsdgpu.h"

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

// rows[c * F + m], c <= M / 2: uniform noise plus a constant 1e3 in row 3; the imaginary parts of rows 0 and M / 2 are not zero
static Veccf rows(int C, int F)
{
  Veccf v(C * F);
  unsigned s = 12345u;
  auto u = [&s] {
    s = s * 1664525u + 1013904223u;
    return (float) ((s >> 8) & 0xffff) / 32768.0f - 1.0f;
  };
  for (int c = 0; c < C; c++)
    for (int m = 0; m < F; m++) {
      const float re = u(), im = u();
      v(c * F + m) = cfloat(re + (c == 3 ? 1e3f : 0.f), im);
    }
  return v;
}

// the definition over the whole block (frames before 0 are zeros): F M samples
static std::vector<double> definition(const Veccf &u, const Vecf &f, int M, int F)
{
  const int K = f.rows(), N = M / 2;
  const double PI = 3.14159265358979323846;
  std::vector<double> x((size_t) F * M);
  for (int p = 0; p < F * M; p++) {
    double acc = 0;
    for (int m = 0; m <= p / M; m++) {
      const int k = p - m * M;
      if (k >= K) continue;
      double inner = (double) u(m).real() + ((p & 1) ? -1.0 : 1.0) * (double) u(N * F + m).real();
      for (int c = 1; c < N; c++) {
        const double a = 2 * PI * (double) (((long long) c * p) % M) / M;
        inner += 2.0 * ((double) u(c * F + m).real() * std::cos(a) - (double) u(c * F + m).imag() * std::sin(a));
      }
      acc += (double) f(k) * inner;
    }
    x[p] = acc;
  }
  return x;
}

static void compare(int M, int K, int F1, int F2)
{
  const int F = F1 + F2, C = M / 2 + 1;
  const Vecf f = design_rif_fen(K, "lp", 0.5f / M);
  const Veccf u = rows(C, F);
  const std::vector<double> ref = definition(u, f, M, F);
  double pk = 0;
  for (double r : ref) pk = std::max(pk, std::abs(r));
  auto f_h = tsd_amd::synthetiseur_polyphase_reel(f, M), f_g = tsd_amd::synthetiseur_polyphase_reel(f, M);
  tsdgpu_synthesizer *raw = nullptr;
  CHECK(tsdgpu_synthesizer_create_real(&raw, M, 1, f.data(), K) == 0, "M=%d: the C ABI refused the shape", M);
  if (!raw) return;
  CHECK(tsdgpu_synthesizer_rows(raw) == C && tsdgpu_synthesizer_is_real(raw) == 1, "M=%d: rows / is_real of the C handle", M);
  int m0 = 0;
  for (int b = 0; b < 2; b++) {
    const int nf = b ? F2 : F1, ni = C * nf, no = nf * M;
    Veccf ub(ni);
    Vecf x_h;
    for (int c = 0; c < C; c++)
      for (int m = 0; m < nf; m++) ub(c * nf + m) = u(c * F + m0 + m);
    f_h->step(ub, x_h);
    CHECK(x_h.rows() == no, "M=%d: %d outputs for %d frames", M, (int) x_h.rows(), nf);
    if (x_h.rows() != no) break;
    double e = 0;
    for (int i = 0; i < no; i++) e = std::max(e, std::abs((double) x_h(i) - ref[(size_t) m0 * M + i]));
    CHECK(e <= 1e-5 * pk, "M=%d K=%d step %d (host): %.3g of the peak", M, K, b, e / pk);
    cfloat *du = (cfloat *) tsd_amd::alloue_gpu((size_t) ni * sizeof(cfloat));
    float *dx = (float *) tsd_amd::alloue_gpu((size_t) no * sizeof(float));
    tsd_amd::copie_vers_gpu(du, ub.data(), (size_t) ni * sizeof(cfloat));
    {
      const Veccf ug = Veccf::map(du, ni);
      Vecf xg = Vecf::map(dx, no);
      f_g->step(ug, xg);
      CHECK(xg.data() == dx && xg.est_sur_gpu(), "M=%d: a pre-sized mapped output must be written in place", M);
    }
    Vecf x_g(no);
    tsd_amd::copie_vers_hote(x_g.data(), dx, (size_t) no * sizeof(float));
    tsd_amd::libere_gpu(du);
    tsd_amd::libere_gpu(dx);
    CHECK(std::memcmp(x_g.data(), x_h.data(), (size_t) no * sizeof(float)) == 0, "M=%d: resident and host runs differ, step %d", M, b);
    // the C ABI on the same block, rows strided in the whole block: the same bits
    std::vector<float> x_c(no);
    int64_t got = 0;
    CHECK(tsdgpu_synthesizer_step(raw, u.data() + m0, F, nf, x_c.data(), no, &got, nullptr) == 0 && got == no, "M=%d: C ABI step %d", M, b);
    CHECK(std::memcmp(x_c.data(), x_h.data(), (size_t) no * sizeof(float)) == 0, "M=%d: the adaptor and the C ABI differ, step %d", M, b);
    m0 += nf;
  }
  tsdgpu_synthesizer_destroy(raw);
}

int main()
{
  compare(32, 100, 21, 13);
  bool threw = false;
  try {
    auto f = tsd_amd::synthetiseur_polyphase_reel(design_rif_fen(31, "lp", 0.05f), 32);
    Veccf u(17 * 10 + 1);
    Vecf x;
    f->step(u, x);
  } catch (...) {
    threw = true;
  }
  CHECK(threw, "a vector that is not nb_canaux / 2 + 1 blocks of one length must be refused");
  threw = false;
  try {
    auto f = tsd_amd::synthetiseur_polyphase_reel(design_rif_fen(31, "lp", 0.05f), 8);
  } catch (...) {
    threw = true;
  }
  CHECK(threw, "a frame length the real-output synthesizer does not serve must be refused by the factory");
  if (nfail) {
    printf("%d failure(s)\n", nfail);
    return 1;
  }
  printf("test_synthetiseur_reel OK\n");
  return 0;
}
