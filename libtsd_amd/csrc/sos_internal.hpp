// sos_internal.hpp -- the block-parallel SOS cascade shared by the single-stream handle (sos.hip) and the channel bank
// (bank.hip): section tables, the running-state layout, the per-wave cascade pass and the handle itself.
#pragma once
#include "common.hpp"
#include <vector>

namespace tsdgpu {

constexpr int SOS_MAX_SEC = 32;
constexpr int LANE_FLOATS = 32;                   // floats a lane holds per sub-tile (16 was measured: twice the scans and LDS work per sample)
constexpr int SUB_FLOATS = 64 * LANE_FLOATS;      // floats per sub-tile (2048)
constexpr int LDS_LANE_PITCH = LANE_FLOATS + 4;   // floats: + 4 pad -> conflict-free b128 both ways (36: 9 x 16 B, odd; 20: 5 x 16 B, odd)
constexpr int LANE_QUADS = LANE_FLOATS / 4;
// float offset of float p (a multiple of 4) of a sub-tile in the wave's LDS image; row = the lane that owns it
__device__ __forceinline__ int sos_img(int p)
{
  return (p / LANE_FLOATS) * LDS_LANE_PITCH + (p % LANE_FLOATS);
}

constexpr int SOS_WARM_FACTOR = 4;    // a chunk is at least this many times its warm-up's cost long
constexpr int NARROW_FLOATS = 4;      // floats per lane of a warm-up step (one 16-B load, no transposition)

struct SosSection {
  float b0, b1, b2, a1, a2;
  float seed;                 // 1: first-sample seed (SOIS), 0: zero start (RIIFoS)
  float df1;                  // 1: FormeDirecte1 (filtre-rt.cc:384-393), 0: FormeDirecte2 (:369-380)
  float sg;                   // +1 / -1: the scans carry (d1, delta = d1 - sg d2) instead of (d1, d2), see sos_cascade
  float A[6][4];              // T (M^L)^(2^k) T^-1, k = 0..5, row-major 2x2, M = [[-a1,-a2],[1,0]], T = [[1,0],[1,-sg]]
  float c1[LANE_FLOATS];      // output response to start state (d1, delta) = (1, 0) (per in-lane sample index)
  float c2[LANE_FLOATS];      // output response to start state (d1, delta) = (0, 1)
  // the same tables for the narrow warm-up steps (L = NARROW_FLOATS / channels samples per lane)
  float An[6][4];
  float c1n[NARROW_FLOATS], c2n[NARROW_FLOATS];
  // Levels of the Kogge-Stone scan that matter: after K levels a lane's sum holds the terms of the 2^K lanes before it, and
  // the first term left out is (M^L)^(2^K) Z = A[K] Z -- below SCAN_TAIL_BOUND of the states for a damped section long before the sixth
  // level (pole radius 0.88: three levels; 0.67: two; 0.5 and less: one).  (The chunk warm-ups use STATE_TAIL_BOUND, common.hpp.)
  int nlev, nlevn;
};

// state buffer layout (floats): [0] = seeded flag, then per (section, channel) four values:
// DF2: (d1, d2, -, -);  DF1: (y1, y2, x1, x2)
__host__ __device__ inline int state_index(int sec, int ch) { return 1 + (sec * 2 + ch) * 4; }
constexpr int STATE_FLOATS = 1 + SOS_MAX_SEC * 8;

__device__ __forceinline__ void wave_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The stream state of the handle is the reference's: per (section, channel) (d1, d2, x1, x2).  The running image a wave keeps
// in LDS holds (d1, delta = d1 - sg d2, x1, x2) -- the coordinates of the scans, see sos_cascade.
__device__ __forceinline__ void state_load(float *sst, const float *__restrict__ st, const SosSection *__restrict__ sec, int nsec, int lane)
{
  for (int i = lane; i < nsec * 8; i += 64) {
    float v = st[1 + i];
    if ((i & 3) == 1) v = st[i] - sec[i >> 3].sg * v;
    sst[i] = v;
  }
}
__device__ __forceinline__ void state_store(float *__restrict__ st, const float *sst, const SosSection *__restrict__ sec, int nsec, int lane)
{
  if (lane == 0) st[0] = 1.f;
  for (int i = lane; i < nsec * 8; i += 64) st[1 + i] = (i & 3) == 1 ? sec[i >> 3].sg * (sst[i - 1] - sst[i]) : sst[i];
}

// One cascade pass over the wave's samples held in registers: lane l owns LF consecutive floats
// (LF / NCH samples per channel), v in, v out.  Per section: zero-state run, Kogge-Stone scan of the
// end states over the 64 lanes, zero-input correction of every sample; the running state of every
// (section, channel) lives in sst (LDS) and is advanced to the end of these 64 * LF floats.
// NARROW selects the tables of the NARROW_FLOATS-per-lane warm-up steps.
// Coordinates of the carried state: (d1, delta = d1 - sg d2), sg = the sign of the poles' real part.  A narrow-band
// section has its poles next to +1 (or -1): M^n ~ [[n+1, -n], [n, -(n-1)]], and a DC level of 10^6 in (d1, d2) -- what
// a cut-off of 1e-4 makes of an offset of 0.5 -- went through the scan as the difference of products of 10^9: the
// states came out with an absolute error of ~100 where the sequential recurrence has 0.1 (outputs 10-25 x noisier than
// the reference's own float32 run against float64).  In (level, slope) coordinates the same maps are
// ~[[1, n], [~0, 1]]: no cancellation.  The zero-state run of a lane produces moderate values, so its delta is exact.
template <int NCH, int LF, bool NARROW>
__device__ __forceinline__ void sos_cascade(float (&v)[LF], const SosSection *__restrict__ sec, int nsec, float *sst, int lane,
                                            bool do_seed, int last = 63)
{
  // `last`: the lane whose end state is carried on (63; a partial sub-tile of the ragged end stops at an earlier lane)
  constexpr int L = LF / NCH;
#pragma unroll 1
  for (int s = 0; s < nsec; s++) {
    const SosSection &k = sec[s];
    const float b0 = k.b0, b1 = k.b1, b2 = k.b2, a1 = k.a1, a2 = k.a2;
    // (the scan's tables loaded here, beside the coefficients -- one scalar-cache round trip for both; read level by level
    // inside the scan, each level waited for its own)
    float A[6][4];
    {
      const float(*Ag)[4] = NARROW ? k.An : k.A;
#pragma unroll
      for (int q = 0; q < 6; q++)
#pragma unroll
        for (int j = 0; j < 4; j++) A[q][j] = Ag[q][j];
    }
    const float *c1 = NARROW ? k.c1n : k.c1, *c2 = NARROW ? k.c2n : k.c2;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      float *ss = &sst[(s * 2 + c) * 4];
      float sin1 = ss[0], sin0 = ss[1];
      float xin1 = ss[2], xin2 = ss[3];                      // DF1 only: previous two inputs
      if (do_seed && k.seed != 0.f) {
        // premier_appel: every memory of the section = its own first input (filtre-rt.cc:361-365)
        const float x0 = __shfl(v[c], 0);
        sin1 = xin1 = xin2 = x0;
        sin0 = x0 - k.sg * x0;
      }
      float d1 = 0.f, d2 = 0.f;
      if (k.df1 == 0.f) {
        // DF2 zero-state run over the lane's L samples (b0 = 1 -- what the pole / zero pairing of
        // filtre_sois always produces -- saves the multiply; same value, 1.0f * d being exact)
        if (b0 == 1.f) {
#pragma unroll
          for (int i = 0; i < L; i++) {
            const float xin = v[i * NCH + c];
            const float d = fmaf(-a2, d2, fmaf(-a1, d1, xin));
            v[i * NCH + c] = fmaf(b2, d2, fmaf(b1, d1, d));
            d2 = d1;
            d1 = d;
          }
        } else {
#pragma unroll
          for (int i = 0; i < L; i++) {
            const float xin = v[i * NCH + c];
            const float d = fmaf(-a2, d2, fmaf(-a1, d1, xin));
            v[i * NCH + c] = fmaf(b2, d2, fmaf(b1, d1, b0 * d));
            d2 = d1;
            d1 = d;
          }
        }
      } else {
        // DF1: v = b0 x + b1 x[-1] + b2 x[-2] (previous lane's last two inputs for i < 2),
        // then the all-pole recursion y = v - a1 y1 - a2 y2 from zero state
        static_assert(L >= 2, "a lane holds at least two samples per channel");
        const float my1 = v[(L - 1) * NCH + c], my2 = v[(L - 2) * NCH + c];
        float xp1 = __shfl_up(my1, 1), xp2 = __shfl_up(my2, 1);
        if (lane == 0) { xp1 = xin1; xp2 = xin2; }
        if (lane == last) { ss[2] = my1; ss[3] = my2; }
#pragma unroll
        for (int i = 0; i < L; i++) {
          const float xin = v[i * NCH + c];
          const float fir = fmaf(b2, xp2, fmaf(b1, xp1, b0 * xin));
          const float yv = fmaf(-a2, d2, fmaf(-a1, d1, fir));
          v[i * NCH + c] = yv;
          xp2 = xp1;
          xp1 = xin;
          d2 = d1;
          d1 = yv;
        }
      }
      // lane 0 absorbs the start state: P = M^L * S_in + Z
      float p1 = d1, p0 = fmaf(-k.sg, d2, d1);
      if (lane == 0) {
        p1 = fmaf(A[0][0], sin1, fmaf(A[0][1], sin0, p1));
        p0 = fmaf(A[0][2], sin1, fmaf(A[0][3], sin0, p0));
      }
      // inclusive Kogge-Stone scan over the 64 lanes: P_l = sum_j (M^L)^(l-j) Z_j, cut where the powers have died out (nlev)
      const int nlev = NARROW ? k.nlevn : k.nlev;
#pragma unroll
      for (int kk = 0; kk < 6; kk++) {
        if (kk >= nlev) break;
        const int dd = 1 << kk;
        const float q1 = __shfl_up(p1, dd), q0 = __shfl_up(p0, dd);
        if (lane >= dd) {
          p1 = fmaf(A[kk][0], q1, fmaf(A[kk][1], q0, p1));
          p0 = fmaf(A[kk][2], q1, fmaf(A[kk][3], q0, p0));
        }
      }
      // true start state of this lane = end state of the previous lane
      float s1 = __shfl_up(p1, 1), s0 = __shfl_up(p0, 1);
      if (lane == 0) { s1 = sin1; s0 = sin0; }
      // zero-input correction of every output of the lane
#pragma unroll
      for (int i = 0; i < L; i++) v[i * NCH + c] = fmaf(c1[i], s1, fmaf(c2[i], s0, v[i * NCH + c]));
      // state after the last sample, carried on
      if (lane == last) {
        ss[0] = p1;
        ss[1] = p0;
      }
    }
    wave_sync();
  }
}

constexpr int SOS_WPE = 4;            // waves per SIMD the kernel is compiled for (a fifth costs spills: profiles/EXPERIMENTS.md)

}  // namespace tsdgpu

struct tsdgpu_sos {
  int data_type = 0, nsec = 0, nch = 1;
  float gain = 1.f;
  tsdgpu::SosSection *d_sec = nullptr;
  float *d_state[2] = {nullptr, nullptr};
  int cur = 0;
  bool capturable = false;      // tsdgpu_sos_set_capturable: the state is back in d_state[0] after every step
  int64_t halo = 0;             // W: samples after which the state transition is below STATE_TAIL_BOUND
  int64_t skip_f = 0;           // tsdgpu_sos_step_skip: floats at the start of the current call that are filtered but not stored
  tsdgpu::DevBuf in_stage, out_stage;
  // exact carry of the state from chunk to chunk (long-memory filters, see sos_kernel)
  int comps = 2;                // state values per section and channel in the carry: 2 (DF2 chain) or 4 (a DF1 section: + its last two inputs)
  std::vector<double> phi;      // one-step zero-input transition of the whole cascade, m x m, m = comps x nsec
  std::vector<float> sg_host;   // per section: the sign of the scans' coordinates (tsdgpu::SosSection::sg)
  tsdgpu::DevBuf carry, scan_ws, scan_P;
  int64_t scan_L = 0;           // the chunk length (samples) scan_P was made for (< 0: no tables for that length)
};

namespace tsdgpu {
int sos_create_ex(tsdgpu_sos **out, int data_type, const float *coefs_host, int nsec, float gain,
                  const float *rii1_host, int forme, int seeded);
}  // namespace tsdgpu
