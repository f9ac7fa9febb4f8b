// synthesizer_real.hip -- the maximally decimated polyphase synthesis bank with a REAL float32 output: the M / 2 + 1 rows a
// RealChannelizer (channelizer_real.hip) or a bank of M / 2 + 1 channels wrote, back into ONE float stream.
//
//   x[p] = sum_m f[p - m M] ( Re u_0[m] + (-1)^p Re u_N[m] + 2 sum_{0 < c < N} Re( u_c[m] exp(+2 pi i c p / M) ) ),   N = M / 2
// which is the complex synthesizer (synthesizer.hip) on the block extended by the rows M - c = conj(row c): exactly real.  The
// imaginary parts of rows 0 and N are not used.  The frame's M-point inverse transform is done at half the length, the
// untangling of channelizer_real.hip run backwards: with U_c = u_c[m], W = W_M = exp(-2 pi i / M), c < N
//   Z_c = (U_c + conj U_{N-c}) + i conj(W^c) (U_c - conj U_{N-c}),   z = IDFT_N(Z) (unscaled),   w_2j = Re z_j, w_2j+1 = Im z_j
//   x[q M + s] = sum_{j < P} f[j M + s] w_s[q - j],   P = ceil(K / M).
// Every frame keeps a transform of its own (channelizer_real.hip says why).
//
// The kernel is synthesizer_kernel (synthesizer.hip) at N, one position per thread, with another load and another back end:
//  - load: channel-major; an item takes the same two frames of the rows c and N - c, 0 < c < N / 2 (a 128-B segment of each row
//    per 8 lanes), and writes both tangled values Z_c, Z_{N-c} frame-major into the image with re and im swapped (tangle_store);
//    the lone pairs (0 with N; N / 2 with itself) come in a small pass of their own.
//  - transform: s16::transform (N = 16 .. 512), s16::dft8 (N = 8), in line (polybank_tile.hpp says why): forward on swapped
//    values, which is the inverse transform with re and im swapped.
//  - back end: thread (r, s), s < N, reads z_s of the unit's frames, keeps the last P - 1 in registers and runs the oldest-first
//    chains with TWO tap sets, f[j M + 2 s] on the .x lane and f[j M + 2 s + 1] on .y; it stores the 8 bytes x[f M + 2 s],
//    x[f M + 2 s + 1].
// The halo unit per sub-run, the history and the launch are synthesizer_kernel's.  The history is the last P - 1 input frames as
// a packed (N + 1, P - 1) block, the samples as the caller gave them.
// The entry points are synthesizer.hip's; this file is the kernel and its launch.
#include "polybank_host.hpp"
#include "polybank_tile.hpp"

namespace tsdgpu {
namespace {

// R0 in {16, 8, 4, 2}: N = R0 16^a >= 16 through s16::transform; R0 = 0: N = 8 through s16::dft8.  One position per thread.
// N, lgN, FP: the transform length M / 2 and its LDS pitch.  ft: P rows of M taps; TW: W_N^i, i < N / 16; WM: W_M^c, c <= N.
template <int R0, int PP>
__global__ __launch_bounds__(CHAN_NT) void synthesizer_real_kernel(const cpx *__restrict__ u, int64_t ldu, float *__restrict__ x,
                                                                  const float *__restrict__ ft, const cpx *__restrict__ TW,
                                                                  const cpx *__restrict__ WM, int N, int lgN, int FP, int64_t F,
                                                                  int64_t per, const cpx *__restrict__ oh, cpx *__restrict__ nh,
                                                                  int al, int xal)
{
  extern __shared__ __attribute__((aligned(16))) char rsyn_raw[];
  cpx *img = reinterpret_cast<cpx *>(rsyn_raw);
  constexpr int NT = CHAN_NT;
  constexpr int PW = PP - 1, PWA = PW > 0 ? PW : 1;      // the window: the last PW transformed frames of the position
  const int t = threadIdx.x;

  // input frame f of row c <= N: history before 0 (zeros before that); frames from F on are zeros and never reach a stored output
  auto fetch = [&](int c, int64_t f) -> cpx {
    if (f < 0) return PW > 0 && f >= -PW ? oh[c * PW + PW + (int) f] : make_float2(0.f, 0.f);
    return f < F ? u[(int64_t) c * ldu + f] : make_float2(0.f, 0.f);
  };
  // frames f, f + 1 of row c: one 16-B load where the rows allow it
  auto fetch2 = [&](int c, int64_t f, cpx &a, cpx &b) {
    if (al && f >= 0 && f + 1 < F) {
      const float4 q = *reinterpret_cast<const float4 *>(u + (int64_t) c * ldu + f);
      a = make_float2(q.x, q.y);
      b = make_float2(q.z, q.w);
    } else {
      a = fetch(c, f);
      b = fetch(c, f + 1);
    }
  };

  // the new history: per row the last PW frames of (old history ++ u[c][0, F))
  if (blockIdx.x == gridDim.x - 1)
    for (int i = t; i < PW * (N + 1); i += NT) {
      const int c = i / PWA, k = i - c * PWA;
      nh[i] = fetch(c, F - PW + k);
    }

  const SubRun sr = sub_run<1>(t, N, lgN, per);
  const int s = sr.s, r = sr.r;
  cpx g[PP];
  cpx prev[PWA];
#pragma unroll
  for (int p = 0; p < PP; p++) g[p] = *reinterpret_cast<const cpx *>(ft + 2 * (p * N + s));
#pragma unroll
  for (int k = 0; k < PWA; k++) prev[k] = make_float2(0.f, 0.f);

  const int tpt = R0 ? N >> 4 : 1;
  // it = -1: the unit before the sub-run, for its last PW transformed frames only
  for (int64_t it = PW > 0 ? -1 : 0; it < per; it++) {
    // channel-major load: item (k, c, rr) = frames 2k, 2k + 1 of sub-run rr's unit, the rows c and N - c, 0 < c < N / 2;
    // 8 lanes per 128-B segment of a row; two items, four segments, in flight per thread
#pragma unroll 2
    for (int v = 0; v < 4; v++) {
      const TileItem q = tile_item(t + NT * v, N >> 1, lgN - 1, sr.R, per, it);
      if (q.c == 0) continue;
      cpx a0, a1, b0, b1;
      fetch2(q.c, q.f, a0, a1);
      fetch2(N - q.c, q.f, b0, b1);
      const cpx w = WM[q.c];
      cpx *fr = img + (q.rr * 16 + 2 * q.k) * FP;
      const int c0 = s16::pad(q.c), c1 = s16::pad(N - q.c);
      tangle_store(fr + c0, fr + c1, a0, b0, w);
      tangle_store(fr + FP + c0, fr + FP + c1, a1, b1, w);
    }
    // the lone pairs: rows 0 and N into Z_0, row N / 2 into Z_{N/2}; 8 lanes per sub-run each
    // (two passes of the workgroup at N = 8, where 16 R = 1024)
    for (int e = t; e < 16 * sr.R; e += NT) {
      const int mid = e >= 8 * sr.R;
      const TileItem q = tile_item(mid ? e - 8 * sr.R : e, 1, 0, sr.R, per, it);     // (k, rr)
      cpx *fr = img + (q.rr * 16 + 2 * q.k) * FP;
      cpx a0, a1;
      if (mid) {
        fetch2(N >> 1, q.f, a0, a1);
        const int cm = s16::pad(N >> 1);
        fr[cm] = tangle_mid(a0);
        fr[FP + cm] = tangle_mid(a1);
      } else {
        cpx b0, b1;
        fetch2(0, q.f, a0, a1);
        fetch2(N, q.f, b0, b1);
        fr[0] = tangle_edge(a0, b0);
        fr[FP] = tangle_edge(a1, b1);
      }
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
      // z[j + q tpt] in v[q]: back to the places this thread read last
#pragma unroll
      for (int q = 0; q < 16; q++) fr[s16::pad(j + q * tpt)] = v[q];
    }
    __syncthreads();

    // back end: position s of the thread's sub-run, 8 frames at a time
    for (int h = 0; h < 2; h++) {
      cpx cur[8];
      const int64_t f0 = ((sr.u0 + it) * 16) + 8 * h;
      const cpx *src = img + (r * 16 + 8 * h) * FP + s16::pad(s);
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const cpx w = src[k * FP];
        cur[k] = make_float2(w.y, w.x);
      }
      if (it >= 0) {
        float *dst = x + f0 * (2 * N) + 2 * s;
        // x[(f0 + i) M + 2 s] + i x[(f0 + i) M + 2 s + 1] = sum_j g[j] frame(i - j), lane by lane, oldest frame first
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const cpx v = window_chain_pair<PP, 1>(g, prev, cur, i);
          if (f0 + i < F) store_pair(dst + (int64_t) i * (2 * N), v, xal);
        }
      }
      window_shift<PW>(prev, cur);
    }
    __syncthreads();
  }
}

}  // namespace

int syn_real_launch(tsdgpu_synthesizer *c, const cpx *u, int64_t ldu, float *x, int64_t F, hipStream_t st)
{
  // (T = M / 2 <= 512: one position per thread at every served M)
  const int rc = polybank_radix(c->T, [&](auto r0, auto) {
    return polybank_taps(c->P, [&](auto pp) {
      constexpr int R0 = decltype(r0)::value, PP = decltype(pp)::value;
      const PolyLaunch g = polybank_geometry(c, 1, F);
      return polybank_launch(c, "synthesizer", synthesizer_real_kernel<R0, PP>, g, st, u, ldu, x, c->d_tab, c->d_tw, c->d_tw2, c->T, c->lgT, c->FP, F,
                             g.per, (const cpx *) c->hist[c->cur], (cpx *) c->hist[c->cur ^ 1], rows_aligned(u, ldu), stream_aligned(x));
    });
  });
  return rc == POLYBANK_UNSERVED ? set_err(TSDGPU_ERR_UNSUPPORTED, "synthesizer_step: %d taps per channel", c->P) : rc;
}

}  // namespace tsdgpu
