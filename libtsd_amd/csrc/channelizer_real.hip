// channelizer_real.hip -- the maximally decimated polyphase analysis bank for a REAL float32 stream: the M / 2 + 1 rows that
// are not the conjugates of others.
//
//   y_c[m] = sum_k h[k] x[n_m - k] exp(-2 pi i c (n_m - k) / M),  n_m = m M + M - 1,  c <= M / 2
// The branch sums v_s[m] = sum_p g_p[s] x[(m - p) M + s], s < M, are real, so the frame's M-point transform is done at half
// the length, N = M / 2: the frame is read as N complex positions z_j = v_2j + i v_2j+1, Z = DFT_N(z), and with Z[N] = Z[0]
//   E = (Z[c] + conj Z[N - c]) / 2,   O = (Z[c] - conj Z[N - c]) / (2 i),   y_c = E + W_M^c O,   c = 0 .. N.
// Every frame keeps a transform of its own: two frames packed into one M-point transform would make a quiet frame carry the
// rounding of its loud neighbour and tie a frame's bits to where the step was cut.
//
// The kernel is channelizer_kernel (channelizer.hip) at N, with another tap load and another read-back:
//  - front: thread (r, s), s < N, loads the 8 bytes x[f M + 2 s], x[f M + 2 s + 1] as one complex position, keeps the same
//    register window and runs the same oldest-first fma chains with TWO tap sets: g_p[2 s] on the .x lane, g_p[2 s + 1] on .y.
//  - transform: s16::transform (N = 16 .. 512), s16::dft8 (N = 8), in line (polybank_tile.hpp says why).
//  - store: the channel-major read-back untangles rows 0 .. N - 1 on the way out (store_rows_real); row N, the Nyquist row,
//    comes from Z[0] alone in a small pass of its own.  Rows 0 and N are written with an imaginary part of exactly 0.
// The history is the last (P - 1) M FLOAT samples; the last workgroup writes the new one into the other buffer.
// The entry points are channelizer.hip's; this file is the kernel and its launch.
#include "polybank_host.hpp"
#include "polybank_tile.hpp"

namespace tsdgpu {
namespace {

// R0 in {16, 8, 4, 2}: N = R0 16^a >= 16 through s16::transform; R0 = 0: N = 8 through s16::dft8.  One position per thread.
// N, lgN, FP: the transform length M / 2 and its LDS pitch.  gt: P rows of M taps; TW: W_N^i, i < N / 16; WM: W_M^c, c <= N.
template <int R0, int PP>
__global__ __launch_bounds__(CHAN_NT) void channelizer_real_kernel(const float *__restrict__ x, cpx *__restrict__ y, int64_t ldy,
                                                                   const float *__restrict__ gt, const cpx *__restrict__ TW,
                                                                   const cpx *__restrict__ WM, int N, int lgN, int FP, int64_t F,
                                                                   int64_t per, const cpx *__restrict__ oh, cpx *__restrict__ nh,
                                                                   int al, int xal)
{
  extern __shared__ __attribute__((aligned(16))) char rchan_raw[];
  cpx *img = reinterpret_cast<cpx *>(rchan_raw);
  constexpr int NT = CHAN_NT;
  constexpr int PW = PP - 1, PWA = PW > 0 ? PW : 1;      // the window: the last PW samples of the position
  const int t = threadIdx.x;
  const int HW = PW * N;                                 // the history in complex positions
  const int64_t n = F * N;

  // the new history: the last HW positions of (old history ++ x[0, n))
  if (blockIdx.x == gridDim.x - 1)
    for (int i = t; i < HW; i += NT) {
      const int64_t g = n - HW + i;
      nh[i] = g < 0 ? oh[HW + g] : load_pair(x + 2 * g, xal);
    }

  const SubRun sr = sub_run<1>(t, N, lgN, per);
  const int s = sr.s, r = sr.r;
  // frame f of the stream, position s: history before 0; frames from F on (the tail of the last unit, idle sub-runs) read
  // the last frame and are never stored
  auto sample = [&](int64_t f) -> cpx {
    f = min(f, F - 1);
    return f < 0 ? oh[(f + PW) * N + s] : load_pair(x + 2 * (f * N + s), xal);
  };
  cpx g[PP];
  cpx prev[PWA];
#pragma unroll
  for (int p = 0; p < PP; p++) g[p] = *reinterpret_cast<const cpx *>(gt + 2 * (p * N + s));
#pragma unroll
  for (int k = 0; k < PW; k++) prev[k] = sample(sr.u0 * 16 - PW + k);

  const int tpt = R0 ? N >> 4 : 1;
  for (int64_t it = 0; it < per; it++) {
    for (int h = 0; h < 2; h++) {
      cpx cur[8];
      const int64_t f0 = ((sr.u0 + it) << 4) + 8 * h;
#pragma unroll
      for (int k = 0; k < 8; k++) cur[k] = sample(f0 + k);
      cpx *dst = img + (r * 16 + 8 * h) * FP + s16::pad(s);
      // v_2s[f0 + i] + i v_2s+1[f0 + i] = sum_p g[p] frame(i - p), lane by lane, oldest sample first
#pragma unroll
      for (int i = 0; i < 8; i++) dst[i * FP] = window_chain_pair<PP, 1>(g, prev, cur, i);
      window_shift<PW>(prev, cur);
    }
    __syncthreads();

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

int chan_real_launch(tsdgpu_channelizer *c, const float *x, cpx *y, int64_t ldy, int64_t F, hipStream_t st)
{
  // (T = M / 2 <= 512: one position per thread at every served M)
  const int rc = polybank_radix(c->T, [&](auto r0, auto) {
    return polybank_taps(c->P, [&](auto pp) {
      constexpr int R0 = decltype(r0)::value, PP = decltype(pp)::value;
      const PolyLaunch g = polybank_geometry(c, 1, F);
      return polybank_launch(c, "channelizer", channelizer_real_kernel<R0, PP>, g, st, x, y, ldy, c->d_tab, c->d_tw, c->d_tw2, c->T, c->lgT, c->FP, F,
                             g.per, (const cpx *) c->hist[c->cur], (cpx *) c->hist[c->cur ^ 1], rows_aligned(y, ldy), stream_aligned(x));
    });
  });
  return rc == POLYBANK_UNSERVED ? set_err(TSDGPU_ERR_UNSUPPORTED, "channelizer_step: %d taps per channel", c->P) : rc;
}

}  // namespace tsdgpu
