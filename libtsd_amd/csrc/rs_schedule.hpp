// rs_schedule.hpp -- the schedule of the resampler's float32 phase recurrence (resample.hip), host arithmetic only: no HIP header,
// so that tests/cpp/test_rs_schedule_cpu.cc runs it on the CPU under the sanitizers.
//
// Per input the reference does  while (phase < 1) { emit; phase += inc; }  phase -= 1;  with `phase` a float32 (libtsd ra.cc:29-73).
// The schedule depends on the increment alone: it is simulated ONCE per ratio and process -- a checkpoint (phase, outputs so far) every
// RS_CK inputs, Brent's cycle detection on the phase at input boundaries -- and shared by the handles of that ratio (a one-shot
// rééchan() creates a handle per call: without the cache every call replayed up to 8 M sequential steps, tens of ms).  The state space
// is finite, so the sequence becomes periodic (160/147: 3 853 516 inputs <-> 4 194 303 outputs): then any position is a table lookup.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

namespace tsdgpu {

constexpr int RS_CK = 8;                                 // checkpoint spacing (inputs)
// the table grows 8 B per RS_CK inputs until the period is found, and counts outputs in 32 bits: a recurrence whose period
// were not found within RS_SIM_MAX inputs is refused instead of growing on
constexpr int64_t RS_SIM_MAX = (int64_t) 1 << 29;        // inputs (a 256 MiB table); 160/147 needs 8 M
struct RsCk { uint32_t phase_bits; uint32_t cum; };      // cum = outputs before this input (canonical index space)

inline float bits2f(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
inline uint32_t f2bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

// the cycle of the phase sequence: state(i + lambda) = state(i) for i >= mu, opp outputs per period; all zero until it is found
struct RsCycle { int64_t mu = 0, lambda = 0, opp = 0; };
struct RsState { uint32_t phase_bits = 0; int64_t cum = 0; };      // the phase at an input boundary, outputs emitted before it

class RsSchedule {
 public:
  explicit RsSchedule(float inc_) : inc(inc_) {}
  // the schedule of this increment, shared by the process (the 32 most recent ratios; handles keep their own reference)
  static std::shared_ptr<RsSchedule> sched_for(float inc)
  {
    static std::mutex m;
    static std::map<uint32_t, std::shared_ptr<RsSchedule>> cache;
    std::lock_guard<std::mutex> lock(m);
    const uint32_t key = f2bits(inc);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    if (cache.size() >= 32) cache.erase(cache.begin());
    return cache[key] = std::make_shared<RsSchedule>(inc);
  }
  // the state at absolute input index i, the table extended as far as that needs; false when the recurrence is refused
  bool state_at(int64_t i, RsState *s)
  {
    std::lock_guard<std::mutex> lock(mtx);
    extend(i);
    if (failed) return false;
    int64_t ic = i, q = 0;
    if (cyc && i >= c.mu + c.lambda) {
      const int64_t d = i - c.mu;
      q = d / c.lambda;
      ic = c.mu + d % c.lambda;
    }
    float p;
    state_at_canonical(ic, &p, &s->cum);
    s->phase_bits = f2bits(p);
    s->cum += q * c.opp;
    return true;
  }
  RsCycle cycle() { std::lock_guard<std::mutex> lock(mtx); return cyc ? c : RsCycle(); }
  // fn(first, count) on the checkpoints from index a on, for the upload; under the lock (the table grows under any handle of the ratio)
  template <typename FN> auto checkpoints_from(size_t a, FN fn)
  {
    std::lock_guard<std::mutex> lock(mtx);
    a = a < ck.size() ? a : ck.size();
    return fn(ck.data() + a, ck.size() - a);
  }
  bool refused() { std::lock_guard<std::mutex> lock(mtx); return failed; }

 private:
  const float inc;
  std::mutex mtx;
  std::vector<RsCk> ck;       // checkpoints every RS_CK inputs of the canonical sequence
  int64_t sim_i = 0;          // inputs simulated so far (canonical)
  float sim_phase = 0.f;
  int64_t sim_cum = 0;
  // Brent cycle detection on the phase at input boundaries
  uint32_t tort_bits = 0;
  int64_t brent_power = 1, brent_lam = 0;
  bool cyc = false;
  RsCycle c;
  bool failed = false;

  static void sim_one(float &phase, int64_t &cum, float inc)
  {
    // plain binary32 adds (SSE scalar ops; compiled without fast-math or contraction)
    float p = phase;
    while (p < 1.f) { p = p + inc; cum++; }
    p = p - 1.f;
    phase = p;
  }
  void checkpoint() { ck.push_back(RsCk{f2bits(sim_phase), (uint32_t) sim_cum}); }
  // state (phase, outputs before) at canonical input index ic, ic <= sim_i
  void state_at_canonical(int64_t ic, float *phase, int64_t *cum) const
  {
    const RsCk &k = ck[(size_t) (ic / RS_CK)];
    float p = bits2f(k.phase_bits);
    int64_t cu = k.cum;
    for (int64_t s = ic % RS_CK; s > 0; s--) sim_one(p, cu, inc);
    *phase = p;
    *cum = cu;
  }
  // advance the simulation until it covers canonical index `upto` or the cycle is known
  void extend(int64_t upto)
  {
    while (!cyc && !failed && sim_i < upto + RS_CK) {
      if (sim_i >= RS_SIM_MAX || sim_cum >= (int64_t) 0xFFFF0000ll) {
        failed = true;
        return;
      }
      if (sim_i % RS_CK == 0) checkpoint();
      // Brent: compare the state at this input boundary with the tortoise
      const uint32_t bits = f2bits(sim_phase);
      if (sim_i == 0) {
        tort_bits = bits;
      } else {
        brent_lam++;
        if (bits == tort_bits) {
          c.lambda = brent_lam;
          // mu = first index whose state recurs lambda inputs later
          float pa = 0.f, pb;
          int64_t ca = 0, cb;
          state_at_canonical(c.lambda, &pb, &cb);
          int64_t m = 0;
          while (f2bits(pa) != f2bits(pb)) {
            sim_one(pa, ca, inc);
            sim_one(pb, cb, inc);
            m++;
          }
          c.mu = m;
          c.opp = cb - ca;
          cyc = true;
          // make sure the table covers [0, mu + lambda + RS_CK)
          while (sim_i < c.mu + c.lambda + 2 * RS_CK) {
            sim_one(sim_phase, sim_cum, inc);
            sim_i++;
            if (sim_i % RS_CK == 0) checkpoint();
          }
          return;
        }
        if (brent_lam == brent_power) {
          tort_bits = bits;
          brent_power *= 2;
          brent_lam = 0;
        }
      }
      sim_one(sim_phase, sim_cum, inc);
      sim_i++;
    }
  }
};

}  // namespace tsdgpu
