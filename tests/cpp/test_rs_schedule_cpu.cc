// The resampler's phase schedule (libtsd_amd/csrc/rs_schedule.hpp) on the CPU, under the sanitizers: checkpoints, Brent's cycle
// detection, the (mu, lambda, outputs per period) fold and the per-process cache against a literal run of the recurrence
//     while (phase < 1) { phase += inc; cum++; }  phase -= 1;
// in float32.  The index result is promised bit-exactly, so every comparison is of phase BITS and of counts.
#include "../../libtsd_amd/csrc/rs_schedule.hpp"
#include <cstdio>
#include <cstdlib>
#include <thread>

using namespace tsdgpu;

static int fails = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (fails++ < 20) {                                 \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__);  \
        std::printf(__VA_ARGS__);                         \
        std::printf("\n");                                \
      }                                                   \
    }                                                     \
  } while (0)

// the literal recurrence, advanced one input at a time
struct Literal {
  float phase = 0.f, inc;
  int64_t i = 0, cum = 0;
  explicit Literal(float inc_) : inc(inc_) {}
  void to(int64_t pos)
  {
    for (; i < pos; i++) {
      volatile float p = phase;      // (volatile: every add is rounded to binary32 where it stands)
      while (p < 1.f) { p = p + inc; cum++; }
      p = p - 1.f;
      phase = p;
    }
  }
};

struct Case { const char *name; float ratio; int64_t mu, lambda, opp; };

static void check_at(RsSchedule &s, Literal &lit, int64_t pos, const char *name)
{
  lit.to(pos);
  RsState st;
  CHECK(s.state_at(pos, &st), "%s: refused at %lld", name, (long long) pos);
  CHECK(st.phase_bits == f2bits(lit.phase) && st.cum == lit.cum, "%s at %lld: phase %08x cum %lld, literal %08x %lld", name, (long long) pos,
        st.phase_bits, (long long) st.cum, f2bits(lit.phase), (long long) lit.cum);
}

// `threads` as the argument: the cache and the threaded section alone (what the thread-sanitizer build is run for)
int main(int argc, char **argv)
{
  const bool threads_only = argc > 1 && std::strcmp(argv[1], "threads") == 0;
  const Case cases[] = {
      {"160/147", (float) (160.0 / 147.0), 2, 3853516, 4194303}, {"1", 1.f, 0, 1, 1}, {"0.5", 0.5f, 0, 2, 1}, {"1.25", 1.25f, 0, 4, 5},
      {"1.5", 1.5f, 0, 2, 3}, {"2", 2.f, 0, 1, 2}, {"2.5", 2.5f, 0, 2, 5}, {"8", 8.f, 0, 1, 8}, {"1/64", 1.f / 64.f, 0, 64, 1},
      {"0.77", 0.77f, 0, 1361787, 1048576}, {"1.999", 1.999f, 0, 2098701, 4195303}, {"3.1", 3.1f, 0, 362411, 1123474},
  };
  for (const Case &c : cases) {
    if (threads_only) break;
    const float inc = 1.f / c.ratio;
    RsSchedule s(inc);
    Literal lit(inc);
    // every index of the start, the table growing as the positions ask
    for (int64_t pos = 0; pos <= 20000; pos++) check_at(s, lit, pos, c.name);
    // about 200 ascending scattered indices up to 2.5 periods out (the cycle becomes known on the way)
    const int64_t far = c.lambda * 5 / 2 + 3 * RS_CK;
    uint64_t lcg = 12345;
    int64_t pos = 20000;
    const int64_t pas = (far - pos) / 200 + 1;
    while (pos < far) {
      lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
      pos += 1 + (int64_t) ((lcg >> 33) % (uint64_t) (2 * pas));
      check_at(s, lit, pos, c.name);
    }
    // (Brent's tortoise sits at a power of two below 2 max(mu, lambda): by 3 lambda + mu the cycle is known)
    if (3 * c.lambda + c.mu + 1 > lit.i) check_at(s, lit, 3 * c.lambda + c.mu + 1, c.name);
    const RsCycle cy = s.cycle();
    CHECK(cy.mu == c.mu && cy.lambda == c.lambda && cy.opp == c.opp, "%s: cycle (%lld, %lld, %lld), expected (%lld, %lld, %lld)", c.name,
          (long long) cy.mu, (long long) cy.lambda, (long long) cy.opp, (long long) c.mu, (long long) c.lambda, (long long) c.opp);
    CHECK(!s.refused(), "%s: refused", c.name);
    // indices below mu and around the first period's end, asked AFTER the cycle is known
    Literal again(inc);
    for (int64_t p : {(int64_t) 0, (int64_t) 1, c.mu, c.mu + 1, (int64_t) 7, (int64_t) 8, (int64_t) 9, (int64_t) 12345})
      if (p >= again.i) check_at(s, again, p, c.name);
    // the table reaches the end of the first period and two checkpoints more
    auto count = [](const RsCk *, size_t n) { return n; };
    const size_t nck = s.checkpoints_from(0, count);
    CHECK(nck >= (size_t) ((c.mu + c.lambda + 2 * RS_CK) / RS_CK), "%s: %zu checkpoints", c.name, nck);
    CHECK(s.checkpoints_from(nck + 5, count) == 0 && s.checkpoints_from(nck - 1, count) == 1, "%s: checkpoints_from past the end", c.name);
    // the checkpoints are the literal loop's states every RS_CK inputs
    Literal every(inc);
    const bool same = s.checkpoints_from(3, [&](const RsCk *k, size_t n) {
      for (size_t i = 0; i < n && i < 2000; i++) {
        every.to((int64_t) (3 + i) * RS_CK);
        if (k[i].phase_bits != f2bits(every.phase) || k[i].cum != (uint32_t) every.cum) return false;
      }
      return true;
    });
    CHECK(same, "%s: a checkpoint differs from the literal loop", c.name);
  }

  // one object per increment
  {
    auto a = RsSchedule::sched_for(1.f / 1.25f), b = RsSchedule::sched_for(1.f / 1.25f), d = RsSchedule::sched_for(1.f / 1.5f);
    CHECK(a.get() == b.get(), "sched_for: two objects for one increment");
    CHECK(a.get() != d.get(), "sched_for: one object for two increments");
  }

  // position 10^9 = the literal loop's first period, folded
  for (float ratio : {1.f, 2.5f}) {
    const float inc = 1.f / ratio;
    auto s = RsSchedule::sched_for(inc);
    RsState st;
    CHECK(s->state_at(1000000000, &st), "ratio %g: refused at 10^9", (double) ratio);
    const RsCycle cy = s->cycle();
    CHECK(cy.lambda > 0, "ratio %g: no cycle", (double) ratio);
    if (cy.lambda > 0) {
      Literal lit(inc);
      lit.to(cy.mu);
      const int64_t cum_mu = lit.cum;
      lit.to(cy.mu + cy.lambda);
      const int64_t per_period = lit.cum - cum_mu;
      const int64_t d = 1000000000 - cy.mu, q = d / cy.lambda;
      Literal rest(inc);
      rest.to(cy.mu + d % cy.lambda);
      CHECK(st.phase_bits == f2bits(rest.phase) && st.cum == rest.cum + q * per_period, "ratio %g at 10^9: phase %08x cum %lld", (double) ratio,
            st.phase_bits, (long long) st.cum);
    }
  }

  // eight threads on one shared schedule, ascending and descending, against a single-threaded one
  {
    const float inc = 1.f / 3.1f;
    const int NP = 400;
    const int64_t step = 2347;
    RsSchedule lone(inc);
    std::vector<RsState> ref(NP);
    for (int k = 0; k < NP; k++) CHECK(lone.state_at(k * step, &ref[(size_t) k]), "single thread: refused");
    auto shared = RsSchedule::sched_for(inc);
    std::vector<int> bad(8, 0);
    std::vector<std::thread> th;
    for (int t = 0; t < 8; t++)
      th.emplace_back([&, t]() {
        for (int j = 0; j < NP; j++) {
          const int k = (t & 1) ? NP - 1 - j : j;
          RsState st;
          if (!shared->state_at(k * step, &st) || st.phase_bits != ref[(size_t) k].phase_bits || st.cum != ref[(size_t) k].cum) bad[(size_t) t]++;
          (void) shared->cycle();
          (void) shared->checkpoints_from((size_t) k, [](const RsCk *q, size_t n) { return n ? q[n - 1].cum : 0u; });
        }
      });
    for (auto &t : th) t.join();
    for (int t = 0; t < 8; t++) CHECK(bad[(size_t) t] == 0, "thread %d: %d results differ from the single-threaded ones", t, bad[(size_t) t]);
  }

  if (fails) {
    std::printf("%d check(s) failed\n", fails);
    return 1;
  }
  std::printf("RS SCHEDULE OK\n");
  return 0;
}
