// channelizer_os.hip -- the oversampled polyphase analysis bank: M channels, a new frame every D = M / OS samples, OS in {2, 4}.
//
//   y_c[m] = sum_k h[k] x[n_m - k] exp(-2 pi i c (n_m - k) / M),  n_m = m D + D - 1,  c < M
// in the fast form: P = ceil(K / M), h zero-padded to P M, g_p[s] = h[p M + M - 1 - s]; frame m (counted over the whole stream)
// covers the positions a_s = (m + 1) D - M + s, s < M:
//   v_s[m] = sum_{p < P} g_p[s] x[a_s - p M],      y_.[m] = DFT_M(w),  w[a_s mod M] = v_s[m]  (forward, unscaled).
// A step of F frames (n = F D samples) writes F outputs to each of the M rows y + c ldy, as the maximally decimated bank does.
//
// The sibling of channelizer_kernel (channelizer.hip), which stays what it is: the same 512-thread workgroup, 16-frame units,
// R = 512 / M sub-runs, LDS image and pitch, transform and channel-major read-back -- the output side of a tile does not know
// the bank is oversampled: the same functions in both (polybank_tile.hpp), launched through the same host scaffold
// (polybank_host.hpp).  Two kernels, not one with OS = 1: that was slower at small P.  What differs is the front:
//  - addressing: thread (r, s) reads x[(f + 1) D - M + s] for frame f of the step, from the handle's history where that lies
//    before the step (a frame may straddle the two).  Consecutive frames overlap by M - D: a sample is asked for OS times by the
//    same workgroup within a few loads.
//  - window: the samples of position s lie D apart and the chain takes every OS-th, v_s[f] = sum_p g_p[s] w[f - p OS] (w[j] the
//    position's sample in frame j), oldest first, zero-padded taps included: (P - 1) OS older samples beside the 8 current ones,
//    read from memory only where a sub-run starts.
//  - rotation: v_s[f] goes to the slot (s + rot_f) mod M of its frame, rot_f = ((phase + f + 1) D) mod M, phase = the hops the
//    stream consumed before the step, modulo OS.  A half unit starts at a multiple of 8 frames, so frame i of a half has the
//    rotation ((phase + 1 + i) mod OS) D: OS slots per thread, computed once.
//  - load-ahead: where the window takes the kernel over 128 VGPRs, and with them the second workgroup of a CU, the lone workgroup
//    asks for the next unit's samples before the transform of the current one (AHEAD below); measured, DESIGN 3.12.
// The last workgroup writes the new history (the last P M - D samples of old history ++ x) into the other buffer.
// The entry points are channelizer.hip's; this file is the kernel and its launch.
#include "polybank_host.hpp"
#include "polybank_tile.hpp"

namespace tsdgpu {
namespace {

// R0, NPOS as channelizer_kernel; PP = P; OS the oversampling: PP OS <= 16, the window stays within 15 older samples.
template <int R0, int NPOS, int PP, int OS>
__global__ __launch_bounds__(CHAN_NT) void channelizer_os_kernel(const cpx *__restrict__ x, cpx *__restrict__ y, int64_t ldy,
                                                                 const float *__restrict__ gt, const cpx *__restrict__ TW, int M, int lgM,
                                                                 int FP, int64_t F, int64_t per, const cpx *__restrict__ oh,
                                                                 cpx *__restrict__ nh, int al, int phase)
{
  static_assert((OS == 2 || OS == 4) && PP * OS <= 16, "the register window holds at most 15 older samples");
  extern __shared__ __attribute__((aligned(16))) char chan_os_raw[];
  cpx *img = reinterpret_cast<cpx *>(chan_os_raw);
  constexpr int NT = CHAN_NT;
  constexpr int PW = (PP - 1) * OS, PWA = PW > 0 ? PW : 1;      // the window: the position's samples of the last PW frames
  // Where the window costs the second workgroup of a CU anyway (over 128 VGPRs), the lone workgroup has registers to spare and
  // nothing to hide its loads behind: it asks for the next unit's 16 samples before the transform of this one (32 more VGPRs).
  // The same samples through the same chains: the same bits.
  constexpr bool AHEAD = NPOS == 1 && R0 != 0 && R0 != 2 && PW >= (R0 == 16 ? 12 : 10);
  const int t = threadIdx.x;
  const int D = M / OS;
  const int HW = PP * M - D;
  const int64_t n = F * D;

  // the new history: the last HW samples of (old history ++ x[0, n))
  if (blockIdx.x == gridDim.x - 1)
    for (int i = t; i < HW; i += NT) {
      const int64_t g = n - HW + i;
      nh[i] = g < 0 ? oh[HW + g] : x[g];
    }

  const SubRun sr = sub_run<NPOS>(t, M, lgM, per);
  const int s = sr.s, r = sr.r;
  // frame f of the step, position s: sample (f + 1) D - M + s of the step, in the history when negative (never before it: f >=
  // -PW); frames from F on (the tail of the last unit, idle sub-runs) read the last frame and are never stored
  auto sample = [&](int64_t f, int a) -> cpx {
    f = min(f, F - 1);
    const int64_t q = (f + 1) * D - M + s + a * NT;
    return q < 0 ? oh[HW + q] : x[q];
  };
  float g[NPOS][PP];
  cpx prev[NPOS][PWA];
  int slot[NPOS][OS];                                                // of frame i of a half unit: slot[i mod OS]
#pragma unroll
  for (int a = 0; a < NPOS; a++) {
#pragma unroll
    for (int p = 0; p < PP; p++) g[a][p] = gt[p * M + s + a * NT];
#pragma unroll
    for (int k = 0; k < PW; k++) prev[a][k] = sample(sr.u0 * 16 - PW + k, a);
#pragma unroll
    for (int j = 0; j < OS; j++) slot[a][j] = s16::pad((s + a * NT + ((phase + 1 + j) & (OS - 1)) * D) & (M - 1));
  }

  cpx nxt[AHEAD ? 2 : 1][8];                                         // AHEAD: the coming unit's samples, by half
  if (AHEAD) {
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
      for (int k = 0; k < 8; k++) nxt[h][k] = sample((sr.u0 << 4) + 8 * h + k, 0);
  }

  const int tpt = R0 ? M >> 4 : 1;
  for (int64_t it = 0; it < per; it++) {
#pragma unroll
    for (int a = 0; a < NPOS; a++)
      for (int h = 0; h < 2; h++) {
        cpx cur[8];
        const int64_t f0 = ((sr.u0 + it) << 4) + 8 * h;
#pragma unroll
        for (int k = 0; k < 8; k++) cur[k] = AHEAD ? nxt[AHEAD ? h : 0][k] : sample(f0 + k, a);
        cpx *dst = img + (r * 16 + 8 * h) * FP;
        // v_s[f0 + i] = sum_p g[p] frame(i - p OS), oldest sample first
#pragma unroll
        for (int i = 0; i < 8; i++) dst[i * FP + slot[a][i & (OS - 1)]] = window_chain<PP, OS>(g[a], prev[a], cur, i);
        window_shift<PW>(prev[a], cur);
      }
    if (AHEAD && it + 1 < per) {                                      // (nothing is read for a unit the sub-run does not have)
#pragma unroll
      for (int h = 0; h < 2; h++)
#pragma unroll
        for (int k = 0; k < 8; k++) nxt[h][k] = sample(((sr.u0 + it + 1) << 4) + 8 * h + k, 0);
    }
    __syncthreads();

    // from here on the tile is a tile of channelizer_kernel: the transform and the read-back are its own
    if (R0 == 0) {
      // M = 8: two frames per thread, each one dft8 (natural order in, natural order out)
#pragma unroll
      for (int h = 0; h < 2; h++) {
        cpx *fr = img + (t + h * NT) * FP;
        cpx e[8];
#pragma unroll
        for (int q = 0; q < 8; q++) e[q] = fr[q];
        s16::dft8(e);
#pragma unroll
        for (int q = 0; q < 8; q++) fr[q] = e[q];
      }
    } else {
      const int tl = t >> (lgM - 4), j = t & (tpt - 1);
#pragma unroll
      for (int a = 0; a < NPOS; a++) {
        cpx *fr = img + (tl + a * (NT >> (lgM - 4))) * FP;
        cpx v[16];
#pragma unroll
        for (int m = 0; m < 16; m++) v[m] = fr[s16::pad(j + m * tpt)];
        __syncthreads();
        s16::transform<R0 ? R0 : 16>(v, fr, TW, M, j, tpt, [] { __syncthreads(); });
        // X[j + q tpt] in v[q]: back to the places this thread read last
#pragma unroll
        for (int q = 0; q < 16; q++) fr[s16::pad(j + q * tpt)] = v[q];
      }
    }
    __syncthreads();

    store_rows<NPOS>(img, y, ldy, M, lgM, FP, F, per, it, sr.R, al, t);
    __syncthreads();
  }
}

}  // namespace

int chan_os_launch(tsdgpu_channelizer *c, const cpx *x, cpx *y, int64_t ldy, int64_t F, hipStream_t st)
{
  const int rc = polybank_radix(c->T, [&](auto r0, auto npos) {
    return polybank_os_taps(c->OS, c->P, [&](auto pp, auto os) {
      constexpr int R0 = decltype(r0)::value, NPOS = decltype(npos)::value, PP = decltype(pp)::value, OS = decltype(os)::value;
      const PolyLaunch g = polybank_geometry(c, NPOS, F);
      return polybank_launch(c, "channelizer", channelizer_os_kernel<R0, NPOS, PP, OS>, g, st, x, y, ldy, c->d_tab, c->d_tw, c->M, c->lgM, c->FP, F,
                             g.per, (const cpx *) c->hist[c->cur], (cpx *) c->hist[c->cur ^ 1], rows_aligned(y, ldy), c->phase);
    });
  });
  return rc == POLYBANK_UNSERVED ? set_err(TSDGPU_ERR_UNSUPPORTED, "channelizer_step: %d taps per channel at oversampling %d", c->P, c->OS) : rc;
}

}  // namespace tsdgpu
