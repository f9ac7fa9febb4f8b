// test_synthetiseur_reel_os.cc -- the three-argument tsd_amd::synthetiseur_polyphase_reel(h, M, surech) on host vectors and on
// resident (device) vectors against a plain double-precision loop of the definition, with N = M / 2, D = M / surech, rows c = 0 .. N
// and p counted over the whole stream,
//     x[p] = sum_m f[p - m D] ( Re u_0[m] + (-1)^p Re u_N[m] + 2 sum_{0<c<N} Re( u_c[m] exp(+2 pi i c p / M) ) ),
// chunked steps against one step, surech = 1 against the two-argument factory, the bits of the C ABI
// (tsdgpu_synthesizer_create_real_oversampled), and the refusals.  Built and run by tests/test_rsynthesizer_os_cpp_gpu.py.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <exception>
#include <string>
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

// the definition over the whole block (frames before 0 are zeros): F D samples
static std::vector<double> definition(const Veccf &u, const Vecf &f, int M, int D, int F)
{
  const int K = f.rows(), N = M / 2;
  const double PI = 3.14159265358979323846;
  std::vector<double> x((size_t) F * D);
  for (int p = 0; p < F * D; p++) {
    double acc = 0;
    for (int m = 0; m <= p / D; m++) {
      const int k = p - m * D;
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

// the frames [m0, m0 + nf) of the (C, F) block u, packed
static Veccf bloc(const Veccf &u, int C, int F, int m0, int nf)
{
  Veccf ub(C * nf);
  for (int c = 0; c < C; c++)
    for (int m = 0; m < nf; m++) ub(c * nf + m) = u(c * F + m0 + m);
  return ub;
}

static void compare(int M, int OS, int K, int F1, int F2)
{
  const int F = F1 + F2, C = M / 2 + 1, D = M / OS;
  const Vecf f = design_rif_fen(K, "lp", 0.5f / M);
  const Veccf u = rows(C, F);
  const std::vector<double> ref = definition(u, f, M, D, F);
  double pk = 0;
  for (double r : ref) pk = std::max(pk, std::abs(r));
  auto f_h = tsd_amd::synthetiseur_polyphase_reel(f, M, OS), f_g = tsd_amd::synthetiseur_polyphase_reel(f, M, OS);
  tsdgpu_synthesizer *raw = nullptr;
  CHECK(tsdgpu_synthesizer_create_real_oversampled(&raw, M, OS, f.data(), K) == 0, "M=%d OS=%d: the C ABI refused the shape", M, OS);
  if (!raw) return;
  CHECK(tsdgpu_synthesizer_rows(raw) == C && tsdgpu_synthesizer_is_real(raw) == 1 && tsdgpu_synthesizer_hop(raw) == D,
        "M=%d OS=%d: rows / is_real / hop of the C handle", M, OS);
  int m0 = 0;
  for (int b = 0; b < 2; b++) {
    const int nf = b ? F2 : F1, ni = C * nf, no = nf * D;
    const Veccf ub = bloc(u, C, F, m0, nf);
    Vecf x_h;
    f_h->step(ub, x_h);
    CHECK(x_h.rows() == no, "M=%d OS=%d: %d outputs for %d frames", M, OS, (int) x_h.rows(), nf);
    if (x_h.rows() != no) break;
    double e = 0;
    for (int i = 0; i < no; i++) e = std::max(e, std::abs((double) x_h(i) - ref[(size_t) m0 * D + i]));
    CHECK(e <= 1e-5 * pk, "M=%d OS=%d K=%d step %d (host): %.3g of the peak", M, OS, K, b, e / pk);
    cfloat *du = (cfloat *) tsd_amd::alloue_gpu((size_t) ni * sizeof(cfloat));
    float *dx = (float *) tsd_amd::alloue_gpu((size_t) no * sizeof(float));
    tsd_amd::copie_vers_gpu(du, ub.data(), (size_t) ni * sizeof(cfloat));
    {
      const Veccf ug = Veccf::map(du, ni);
      Vecf xg = Vecf::map(dx, no);
      f_g->step(ug, xg);
      CHECK(xg.data() == dx && xg.est_sur_gpu(), "M=%d OS=%d: a pre-sized mapped output must be written in place", M, OS);
    }
    Vecf x_g(no);
    tsd_amd::copie_vers_hote(x_g.data(), dx, (size_t) no * sizeof(float));
    tsd_amd::libere_gpu(du);
    tsd_amd::libere_gpu(dx);
    CHECK(std::memcmp(x_g.data(), x_h.data(), (size_t) no * sizeof(float)) == 0, "M=%d OS=%d: resident and host runs differ, step %d", M, OS,
          b);
    // the C ABI on the same block, rows strided in the whole block: the same bits
    std::vector<float> x_c(no);
    int64_t got = 0;
    CHECK(tsdgpu_synthesizer_step(raw, u.data() + m0, F, nf, x_c.data(), no, &got, nullptr) == 0 && got == no, "M=%d OS=%d: C ABI step %d", M,
          OS, b);
    CHECK(std::memcmp(x_c.data(), x_h.data(), (size_t) no * sizeof(float)) == 0, "M=%d OS=%d: the adaptor and the C ABI differ, step %d", M, OS,
          b);
    m0 += nf;
    CHECK(tsdgpu_synthesizer_get_phase(raw) == m0 % OS, "M=%d OS=%d: the phase after %d frames", M, OS, m0);
  }
  tsdgpu_synthesizer_destroy(raw);
}

// one step of F frames against steps of 1, 7, 5 and the rest (odd counts: the phase moves), bit for bit
static void chunked(int M, int OS, int K, int F)
{
  const int C = M / 2 + 1, D = M / OS;
  const Vecf f = design_rif_fen(K, "lp", 0.5f / M);
  const Veccf u = rows(C, F);
  auto one = tsd_amd::synthetiseur_polyphase_reel(f, M, OS), many = tsd_amd::synthetiseur_polyphase_reel(f, M, OS);
  Vecf x1;
  one->step(u, x1);
  CHECK(x1.rows() == F * D, "M=%d OS=%d: %d outputs for %d frames", M, OS, (int) x1.rows(), F);
  if (x1.rows() != F * D) return;
  const int cuts[4] = {1, 7, 5, F - 13};
  int m0 = 0;
  for (int b = 0; b < 4; b++) {
    Vecf xb;
    many->step(bloc(u, C, F, m0, cuts[b]), xb);
    CHECK(xb.rows() == cuts[b] * D && std::memcmp(xb.data(), &x1(m0 * D), (size_t) cuts[b] * D * sizeof(float)) == 0,
          "M=%d OS=%d: chunk %d differs from the single step", M, OS, b);
    m0 += cuts[b];
  }
}

// surech = 1 is the two-argument factory, bit for bit
static void surech_un(int M, int K, int F)
{
  const int C = M / 2 + 1;
  const Vecf f = design_rif_fen(K, "lp", 0.5f / M);
  const Veccf u = rows(C, F);
  auto a = tsd_amd::synthetiseur_polyphase_reel(f, M), b = tsd_amd::synthetiseur_polyphase_reel(f, M, 1);
  for (int s = 0; s < 2; s++) {
    const int m0 = s ? 9 : 0, nf = s ? F - 9 : 9;
    Vecf xa, xb;
    a->step(bloc(u, C, F, m0, nf), xa);
    b->step(bloc(u, C, F, m0, nf), xb);
    CHECK(xa.rows() == nf * M && xa.rows() == xb.rows() && std::memcmp(xa.data(), xb.data(), (size_t) xa.rows() * sizeof(float)) == 0,
          "M=%d: surech = 1 differs from the two-argument factory, step %d", M, s);
  }
}

template <typename FN> static std::string texte_echec(FN fn)
{
  try {
    fn();
  } catch (const std::exception &e) {
    return std::string("!") + e.what();
  } catch (...) {
    return "!";
  }
  return "";
}

int main()
{
  compare(32, 2, 100, 21, 13);
  compare(64, 4, 150, 7, 12);
  chunked(32, 2, 100, 40);
  chunked(64, 4, 16 * 16, 40);
  surech_un(32, 100, 20);
  std::string t = texte_echec([] {
    auto f = tsd_amd::synthetiseur_polyphase_reel(design_rif_fen(31, "lp", 0.05f), 32, 2);
    Veccf u(17 * 10 + 1);
    Vecf x;
    f->step(u, x);
  });
  CHECK(!t.empty(), "a vector that is not nb_canaux / 2 + 1 blocks of one length must be refused");
  CHECK(t.find("blocks") != std::string::npos && t.find("17") != std::string::npos, "the refusal names the rows: '%s'", t.c_str());
  t = texte_echec([] {
    auto f = tsd_amd::synthetiseur_polyphase_reel(design_rif_fen(31, "lp", 0.05f), 32, 2);
    Veccf u(17 * 3);
    Vecf x;
    f->step(u, x);
    if (x.rows() != 16 * 3) throw std::runtime_error("three frames must give 3 hops of 16 floats");
  });
  CHECK(t.empty(), "three frames must be served: '%s'", t.c_str());
  t = texte_echec([] { auto f = tsd_amd::synthetiseur_polyphase_reel(design_rif_fen(31, "lp", 0.05f), 32, 0); });
  CHECK(!t.empty(), "surech = 0 must be refused by the factory");
  CHECK(t.find("surech") != std::string::npos, "the refusal names surech: '%s'", t.c_str());
  t = texte_echec([] { auto f = tsd_amd::synthetiseur_polyphase_reel(design_rif_fen(31, "lp", 0.05f), 32, 3); });
  CHECK(!t.empty(), "surech = 3 must be refused by the factory");
  CHECK(t.find("oversample") != std::string::npos, "the refusal carries the C ABI's message: '%s'", t.c_str());
  t = texte_echec([] { auto f = tsd_amd::synthetiseur_polyphase_reel(design_rif_fen(31, "lp", 0.05f), 8, 2); });
  CHECK(!t.empty(), "a frame length the bank does not serve must be refused by the factory");
  if (nfail) {
    printf("%d failure(s)\n", nfail);
    return 1;
  }
  printf("test_synthetiseur_reel_os OK\n");
  return 0;
}
