// channelizer_real_os.hip -- the oversampled polyphase analysis bank for a REAL float32 stream: M / 2 + 1 rows, a new frame
// every D = M / OS floats, OS in {2, 4}.
//
//   y_c[m] = sum_k h[k] x[n_m - k] exp(-2 pi i c (n_m - k) / M),  n_m = m D + D - 1,  c <= M / 2
// the rows 0 .. M / 2 of channelizer_os.hip's bank on the widened stream.  It is to channelizer_real_kernel
// (channelizer_real.hip) what channelizer_os_kernel is to channelizer_kernel: the same half-length transform N = M / 2 of the
// frame's even / odd packing, the same untangling read-back (store_rows_real) and Nyquist pass -- the output side does not know
// the bank is oversampled -- and the front of channelizer_os.hip expressed in complex positions:
//  - addressing: D is even at every served shape (M >= 16, OS <= 4), D2 = D / 2.  Thread (r, s), s < N, reads the pair at float
//    index 2 ((f + 1) D2 - N + s) of the step for frame f, from the handle's history where that is negative.  The history
//    P M - D is even: a pair never straddles history and x.  8-B loads where x is 8-B aligned, two 4-B loads where not.
//  - window: the position's pairs lie D floats apart and the chain takes every OS-th, oldest first, zero-padded taps included,
//    with two tap sets, g_p[2 s] on .x and g_p[2 s + 1] on .y: (P - 1) OS older pairs beside the 8 current ones, read from
//    memory only where a sub-run starts.
//  - rotation: the frame's rotation ((m + 1) D) mod M is even, so pairs stay pairs: the pair of position s goes to the slot
//    (s + rot2) mod N, rot2 = (((phase + 1 + i) mod OS) D2) mod N for frame i of a half unit: OS slots per thread, computed once.
//  - load-ahead: where the registers cost the second workgroup of a CU anyway, the lone workgroup asks for the next unit's
//    pairs before the transform of the current one (AHEAD below); measured, DESIGN 3.16.
// The last workgroup writes the new history (the last P M - D floats of old history ++ x) into the other buffer.
// The entry points are channelizer.hip's; this file is the kernel and its launch.
#include "polybank_host.hpp"
#include "polybank_tile.hpp"

namespace tsdgpu {
namespace {

// R0, N, lgN, FP, gt, TW, WM as channelizer_real_kernel; PP = P; OS the oversampling: PP OS <= 16, the window stays within 15
// older pairs.  oh, nh: the history as P N - D2 pairs.
template <int R0, int PP, int OS>
__global__ __launch_bounds__(CHAN_NT) void channelizer_real_os_kernel(const float *__restrict__ x, cpx *__restrict__ y, int64_t ldy,
                                                                      const float *__restrict__ gt, const cpx *__restrict__ TW,
                                                                      const cpx *__restrict__ WM, int N, int lgN, int FP, int64_t F,
                                                                      int64_t per, const cpx *__restrict__ oh, cpx *__restrict__ nh,
                                                                      int al, int xal, int phase)
{
  static_assert((OS == 2 || OS == 4) && PP * OS <= 16, "the register window holds at most 15 older pairs");
  extern __shared__ __attribute__((aligned(16))) char rchan_os_raw[];
  cpx *img = reinterpret_cast<cpx *>(rchan_os_raw);
  constexpr int NT = CHAN_NT;
  constexpr int PW = (PP - 1) * OS, PWA = PW > 0 ? PW : 1;      // the window: the position's pairs of the last PW frames
  // Where the kernel is over 128 VGPRs anyway (R0 = 2 at every P; the window elsewhere), the lone workgroup of a CU asks for the
  // next unit's 16 pairs before the transform of this one (32 more VGPRs), as channelizer_os_kernel does.  The same pairs
  // through the same chains: the same bits.  Measured, DESIGN 3.16.
  constexpr bool AHEAD = R0 == 2 || (R0 != 0 && PW >= (R0 == 16 ? (OS == 2 ? 8 : 12) : R0 == 8 ? 8 : 6));
  const int t = threadIdx.x;
  const int D2 = N / OS;                                        // the hop in pairs
  const int HW = PP * N - D2;                                   // the history in pairs
  const int64_t n = F * D2;

  // the new history: the last HW pairs of (old history ++ x[0, 2 n))
  if (blockIdx.x == gridDim.x - 1)
    for (int i = t; i < HW; i += NT) {
      const int64_t g = n - HW + i;
      nh[i] = g < 0 ? oh[HW + g] : load_pair(x + 2 * g, xal);
    }

  const SubRun sr = sub_run<1>(t, N, lgN, per);
  const int s = sr.s, r = sr.r;
  // frame f of the step, position s: pair (f + 1) D2 - N + s of the step, in the history when negative (never before it: f >=
  // -PW); frames from F on (the tail of the last unit, idle sub-runs) read the last frame and are never stored
  auto sample = [&](int64_t f) -> cpx {
    f = min(f, F - 1);
    const int64_t q = (f + 1) * D2 - N + s;
    return q < 0 ? oh[HW + q] : load_pair(x + 2 * q, xal);
  };
  cpx g[PP];
  cpx prev[PWA];
  int slot[OS];                                                  // of frame i of a half unit: slot[i mod OS]
#pragma unroll
  for (int p = 0; p < PP; p++) g[p] = *reinterpret_cast<const cpx *>(gt + 2 * (p * N + s));
#pragma unroll
  for (int k = 0; k < PW; k++) prev[k] = sample(sr.u0 * 16 - PW + k);
#pragma unroll
  for (int j = 0; j < OS; j++) slot[j] = s16::pad((s + ((phase + 1 + j) & (OS - 1)) * D2) & (N - 1));

  cpx nxt[AHEAD ? 2 : 1][8];                                     // AHEAD: the coming unit's pairs, by half
  if (AHEAD) {
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
      for (int k = 0; k < 8; k++) nxt[h][k] = sample((sr.u0 << 4) + 8 * h + k);
  }

  const int tpt = R0 ? N >> 4 : 1;
  for (int64_t it = 0; it < per; it++) {
    for (int h = 0; h < 2; h++) {
      cpx cur[8];
      const int64_t f0 = ((sr.u0 + it) << 4) + 8 * h;
#pragma unroll
      for (int k = 0; k < 8; k++) cur[k] = AHEAD ? nxt[AHEAD ? h : 0][k] : sample(f0 + k);
      cpx *dst = img + (r * 16 + 8 * h) * FP;
      // v_2s[f0 + i] + i v_2s+1[f0 + i] = sum_p g[p] frame(i - p OS), lane by lane, oldest sample first
#pragma unroll
      for (int i = 0; i < 8; i++) dst[i * FP + slot[i & (OS - 1)]] = window_chain_pair<PP, OS>(g, prev, cur, i);
      window_shift<PW>(prev, cur);
    }
    if (AHEAD && it + 1 < per) {                                  // (nothing is read for a unit the sub-run does not have)
#pragma unroll
      for (int h = 0; h < 2; h++)
#pragma unroll
        for (int k = 0; k < 8; k++) nxt[h][k] = sample(((sr.u0 + it + 1) << 4) + 8 * h + k);
    }
    __syncthreads();

    // from here on the tile is a tile of channelizer_real_kernel: the transform and the read-back are its own
    if (R0 == 0) {
      // N = 8: two frames per thread, each one dft8 (natural order in, natural order out)
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
      const int tl = t >> (lgN - 4), j = t & (tpt - 1);
      cpx *fr = img + tl * FP;
      cpx v[16];
#pragma unroll
      for (int m = 0; m < 16; m++) v[m] = fr[s16::pad(j + m * tpt)];
      __syncthreads();
      s16::transform<R0 ? R0 : 16>(v, fr, TW, N, j, tpt, [] { __syncthreads(); });
      // Z[j + q tpt] in v[q]: back to the places this thread read last
#pragma unroll
      for (int q = 0; q < 16; q++) fr[s16::pad(j + q * tpt)] = v[q];
    }
    __syncthreads();

    store_rows_real(img, y, ldy, WM, N, lgN, FP, F, per, it, sr.R, al, t);
    __syncthreads();
  }
}

}  // namespace

int chan_real_os_launch(tsdgpu_channelizer *c, const float *x, cpx *y, int64_t ldy, int64_t F, hipStream_t st)
{
  // (T = M / 2 <= 512: one position per thread at every served M)
  const int rc = polybank_radix(c->T, [&](auto r0, auto) {
    return polybank_os_taps(c->OS, c->P, [&](auto pp, auto os) {
      constexpr int R0 = decltype(r0)::value, PP = decltype(pp)::value, OS = decltype(os)::value;
      const PolyLaunch g = polybank_geometry(c, 1, F);
      return polybank_launch(c, "channelizer", channelizer_real_os_kernel<R0, PP, OS>, g, st, x, y, ldy, c->d_tab, c->d_tw, c->d_tw2, c->T, c->lgT,
                             c->FP, F, g.per, (const cpx *) c->hist[c->cur], (cpx *) c->hist[c->cur ^ 1], rows_aligned(y, ldy),
                             stream_aligned(x), c->phase);
    });
  });
  return rc == POLYBANK_UNSERVED ? set_err(TSDGPU_ERR_UNSUPPORTED, "channelizer_step: %d taps per channel at oversampling %d", c->P, c->OS) : rc;
}

}  // namespace tsdgpu
