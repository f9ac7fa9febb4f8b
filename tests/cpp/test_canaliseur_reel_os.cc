// test_canaliseur_reel_os.cc -- the three-argument tsd_amd::canaliseur_polyphase_reel(h, M, surech) on host vectors and on resident
// (device) vectors against a plain double-precision loop of the definition, rows c = 0 .. M / 2 only,
//     y_c[m] = sum_k h[k] x[n_m - k] exp(-2 pi i c (n_m - k) / M),  n_m = m D + D - 1,  D = M / surech,  x real,
// chunked steps against one step, surech = 1 against the two-argument factory, and the refusals.  Built and run by
// tests/test_rchannelizer_os_cpp_gpu.py.
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
static std::vector<cd> definition(const Vecf &x, const Vecf &h, int M, int D)
{
  const int F = x.rows() / D, K = h.rows(), C = M / 2 + 1;
  const double PI = 3.14159265358979323846;
  std::vector<cd> y((size_t) C * F), w(M);
  for (int i = 0; i < M; i++) w[i] = cd(std::cos(2 * PI * i / M), -std::sin(2 * PI * i / M));
  for (int m = 0; m < F; m++) {
    const int nm = m * D + D - 1;
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

// the hops [m0, m0 + nf) of x through f -> y (host)
static Veccf pas(const sptr<FiltreGen<float, cfloat>> &f, const Vecf &x, int D, int m0, int nf)
{
  Vecf xb(nf * D);
  for (int i = 0; i < nf * D; i++) xb(i) = x(m0 * D + i);
  Veccf y;
  f->step(xb, y);
  return y;
}

static void compare(int M, int OS, int K, int F1, int F2)
{
  const int F = F1 + F2, C = M / 2 + 1, D = M / OS;
  const Vecf h = design_rif_fen(K, "lp", 0.5f / M);
  const Vecf x = signal(F * D, M);
  const std::vector<cd> ref = definition(x, h, M, D);
  auto f_h = tsd_amd::canaliseur_polyphase_reel(h, M, OS), f_g = tsd_amd::canaliseur_polyphase_reel(h, M, OS);
  int m0 = 0;
  for (int b = 0; b < 2; b++) {
    const int nf = b ? F2 : F1, n = nf * D, no = C * nf;
    Vecf xb(n);
    for (int i = 0; i < n; i++) xb(i) = x(m0 * D + i);
    const Veccf y_h = pas(f_h, x, D, m0, nf);
    CHECK(y_h.rows() == no, "M=%d OS=%d: %d outputs for %d samples", M, OS, (int) y_h.rows(), n);
    if (y_h.rows() != no) return;
    const double eh = ecart(y_h.data(), nf, ref, F, C, m0, nf);
    CHECK(eh <= 1e-5, "M=%d OS=%d K=%d step %d (host): %.3g of the peak", M, OS, K, b, eh);
    for (int m = 0; m < nf; m++)
      CHECK(y_h((C - 1) * nf + m).imag() == 0.0f && y_h(m).imag() == 0.0f, "M=%d OS=%d: rows 0 and M / 2 must be exactly real (frame %d)",
            M, OS, m);
    float *dx = (float *) tsd_amd::alloue_gpu((size_t) n * sizeof(float));
    cfloat *dy = (cfloat *) tsd_amd::alloue_gpu((size_t) no * sizeof(cfloat));
    tsd_amd::copie_vers_gpu(dx, xb.data(), (size_t) n * sizeof(float));
    {
      const Vecf xg = Vecf::map(dx, n);
      Veccf yg = Veccf::map(dy, no);
      f_g->step(xg, yg);
      CHECK(yg.data() == dy && yg.est_sur_gpu(), "M=%d OS=%d: a pre-sized mapped output must be written in place", M, OS);
    }
    Veccf y_g(no);
    tsd_amd::copie_vers_hote(y_g.data(), dy, (size_t) no * sizeof(cfloat));
    tsd_amd::libere_gpu(dx);
    tsd_amd::libere_gpu(dy);
    CHECK(std::memcmp(y_g.data(), y_h.data(), (size_t) no * sizeof(cfloat)) == 0, "M=%d OS=%d: resident and host runs differ, step %d", M, OS,
          b);
    m0 += nf;
  }
}

// one step of F hops against steps of 1, 7, 5 and the rest (odd counts: the phase moves), bit for bit
static void chunked(int M, int OS, int K, int F)
{
  const int C = M / 2 + 1, D = M / OS;
  const Vecf h = design_rif_fen(K, "lp", 0.5f / M);
  const Vecf x = signal(F * D, M);
  auto one = tsd_amd::canaliseur_polyphase_reel(h, M, OS), many = tsd_amd::canaliseur_polyphase_reel(h, M, OS);
  const Veccf y1 = pas(one, x, D, 0, F);
  const int cuts[4] = {1, 7, 5, F - 13};
  int m0 = 0;
  for (int b = 0; b < 4; b++) {
    const Veccf yb = pas(many, x, D, m0, cuts[b]);
    for (int c = 0; c < C; c++)
      CHECK(std::memcmp(&yb(c * cuts[b]), &y1(c * F + m0), (size_t) cuts[b] * sizeof(cfloat)) == 0,
            "M=%d OS=%d: chunk %d differs from the single step in row %d", M, OS, b, c);
    m0 += cuts[b];
  }
}

// surech = 1 is the two-argument factory, bit for bit
static void surech_un(int M, int K, int F)
{
  const Vecf h = design_rif_fen(K, "lp", 0.5f / M);
  const Vecf x = signal(F * M, M);
  auto a = tsd_amd::canaliseur_polyphase_reel(h, M), b = tsd_amd::canaliseur_polyphase_reel(h, M, 1);
  for (int s = 0; s < 2; s++) {
    const int m0 = s ? 9 : 0, nf = s ? F - 9 : 9;
    const Veccf ya = pas(a, x, M, m0, nf), yb = pas(b, x, M, m0, nf);
    CHECK(ya.rows() == yb.rows() && std::memcmp(ya.data(), yb.data(), (size_t) ya.rows() * sizeof(cfloat)) == 0,
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
    auto f = tsd_amd::canaliseur_polyphase_reel(design_rif_fen(31, "lp", 0.05f), 32, 2);
    Vecf x(16 * 10 + 1);
    Veccf y;
    f->step(x, y);
  });
  CHECK(!t.empty(), "a vector that is not a whole number of hops must be refused");
  CHECK(t.find("hops") != std::string::npos && t.find("16") != std::string::npos, "the refusal names the hop: '%s'", t.c_str());
  t = texte_echec([] {
    auto f = tsd_amd::canaliseur_polyphase_reel(design_rif_fen(31, "lp", 0.05f), 32, 2);
    Vecf x(32 + 16);                                   // three hops: not whole frames, and served
    Veccf y;
    f->step(x, y);
    if (y.rows() != 17 * 3) throw std::runtime_error("three hops must give 17 x 3 outputs");
  });
  CHECK(t.empty(), "a whole number of hops must be served: '%s'", t.c_str());
  t = texte_echec([] { auto f = tsd_amd::canaliseur_polyphase_reel(design_rif_fen(31, "lp", 0.05f), 32, 0); });
  CHECK(!t.empty(), "surech = 0 must be refused by the factory");
  CHECK(t.find("surech") != std::string::npos, "the refusal names surech: '%s'", t.c_str());
  t = texte_echec([] { auto f = tsd_amd::canaliseur_polyphase_reel(design_rif_fen(31, "lp", 0.05f), 32, 3); });
  CHECK(!t.empty(), "surech = 3 must be refused by the factory");
  CHECK(t.find("oversample") != std::string::npos, "the refusal carries the C ABI's message: '%s'", t.c_str());
  if (nfail) {
    printf("%d failure(s)\n", nfail);
    return 1;
  }
  printf("test_canaliseur_reel_os OK\n");
  return 0;
}
