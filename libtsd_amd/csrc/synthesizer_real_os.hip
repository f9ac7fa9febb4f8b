// synthesizer_real_os.hip -- the oversampled polyphase synthesis bank with a REAL float32 output: the M / 2 + 1 rows an oversampled
// RealChannelizer (channelizer_real_os.hip) or a bank of M / 2 + 1 channels wrote, at hop D = M / OS, OS in {2, 4}, back into ONE
// float stream.
//
//   x[p] = sum_m f[p - m D] ( Re u_0[m] + (-1)^p Re u_N[m] + 2 sum_{0 < c < N} Re( u_c[m] exp(+2 pi i c p / M) ) ),   N = M / 2
// with p counted over the whole stream: the oversampled complex synthesizer (synthesizer_os.hip) on the block extended by the rows
// M - c = conj(row c), exactly real.  The imaginary parts of rows 0 and N are not used.  In the fast form, Q = ceil(K / D), f
// zero-padded to Q D, the frame's M real values w_.[m] from the tangle and the N-point inverse transform of synthesizer_real.hip
// (w_2j = Re z_j, w_2j+1 = Im z_j), and p = q D + s', s' < D:
//   x[q D + s'] = sum_{j < Q} f[j D + s'] w_r[q - j],   r = ((hops0 + q) D + s') mod M: the same position r in all Q frames,
// hops0 the hops the stream consumed before the step (the handle's phase, modulo OS).
// A step of F frames reads F samples from each of the M / 2 + 1 rows u + c ldu and writes n = F D floats of x.
//
// The sibling of synthesizer_real_kernel (synthesizer_real.hip), as synthesizer_os_kernel is synthesizer_kernel's: the input side
// of a tile -- the pair items (c, N - c) through tangle_store, the lone-pair pass, the in-line transform at N, the halo unit where a
// sub-run starts, one position per thread -- does not know the bank is oversampled.  What differs is the back end:
//  - thread s < N still owns the real positions 2 s and 2 s + 1 of the transformed frames and keeps their last Q - 1 pairs in
//    registers.  D is even (D >= 4), so both lie in one hop block: the tap pairs are g[j] = (f[j D + (2 s mod D)], f[.. + 1]), and
//    the pair has an output only at the hops with (phase + q) mod OS = floor(2 s / D).  It is the chain j = Q-1 .. 0 (oldest frame
//    first) and lands at x[q D + (2 s mod D)] and the float after it: one 8-B store where x is 8-B aligned, two 4-B stores where not.
//  - a half unit starts at a multiple of 8 frames and OS divides 8: frame i of a half is owned where (i mod OS) = (floor(2 s / D) -
//    phase) mod OS, the same test in every half, no register indexed at run time.  From D = 128 (64 threads to a hop) the test
//    is wave-uniform and a wave skips the chains it does not own; below, lanes diverge.
// OS and the phase are launch arguments: the instantiations are synthesizer_real_kernel's, <R0, Q>.
// The last workgroup writes the new history (the last Q - 1 input frames of old history ++ u, per row, as fed) into the other
// buffer: a packed (N + 1, Q - 1) block.
// The entry points are synthesizer.hip's; this file is the kernel and its launch.
#include "polybank_host.hpp"
#include "polybank_tile.hpp"

namespace tsdgpu {
namespace {

// R0, N, lgN, FP, ft, TW, WM: as synthesizer_real_kernel's; QQ = Q tap pairs per position; lgOS = 1, 2; phase < OS.
// ft: Q rows of M taps, row j position r taking f[j D + (r mod D)].
template <int R0, int QQ>
__global__ __launch_bounds__(CHAN_NT) void synthesizer_real_os_kernel(const cpx *__restrict__ u, int64_t ldu, float *__restrict__ x,
                                                                     const float *__restrict__ ft, const cpx *__restrict__ TW,
                                                                     const cpx *__restrict__ WM, int N, int lgN, int FP, int64_t F,
                                                                     int64_t per, const cpx *__restrict__ oh, cpx *__restrict__ nh,
                                                                     int al, int xal, int lgOS, int phase)
{
  extern __shared__ __attribute__((aligned(16))) char rsyn_os_raw[];
  cpx *img = reinterpret_cast<cpx *>(rsyn_os_raw);
  constexpr int NT = CHAN_NT;
  constexpr int PW = QQ - 1, PWA = PW > 0 ? PW : 1;      // the window: the last PW transformed frames of the position
  const int t = threadIdx.x;
  const int lgD = lgN + 1 - lgOS, D = 1 << lgD, OSM = (1 << lgOS) - 1;

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
  cpx g[QQ];
  cpx prev[PWA];
#pragma unroll
  for (int p = 0; p < QQ; p++) g[p] = *reinterpret_cast<const cpx *>(ft + 2 * (p * N + s));
#pragma unroll
  for (int k = 0; k < PWA; k++) prev[k] = make_float2(0.f, 0.f);
  const int sel = (((2 * s) >> lgD) - phase) & OSM;      // frame i of a half unit is the pair's where (i mod OS) == sel

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

    // from here to the back end the tile is a tile of synthesizer_real_kernel: the transform is its own
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

    // back end: the pair s of the thread's sub-run, 8 frames at a time
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
        float *dst = x + (f0 << lgD) + ((2 * s) & (D - 1));
        // x[(f0 + i) D + (2 s mod D)] + i x[.. + 1] = sum_j g[j] frame(i - j), lane by lane, oldest frame first, at the hops the
        // pair owns
#pragma unroll
        for (int i = 0; i < 8; i++)
          if ((i & OSM) == sel) {
            const cpx v = window_chain_pair<QQ, 1>(g, prev, cur, i);
            if (f0 + i < F) store_pair(dst + ((int64_t) i << lgD), v, xal);
          }
      }
      window_shift<PW>(prev, cur);
    }
    __syncthreads();
  }
}

}  // namespace

int syn_real_os_launch(tsdgpu_synthesizer *c, const cpx *u, int64_t ldu, float *x, int64_t F, hipStream_t st)
{
  if (c->OS != 2 && c->OS != 4) return set_err(TSDGPU_ERR_UNSUPPORTED, "synthesizer_step: oversampling %d", c->OS);
  // (T = M / 2 <= 512: one position per thread at every served M)
  const int rc = polybank_radix(c->T, [&](auto r0, auto) {
    return polybank_taps(c->P, [&](auto qq) {
      constexpr int R0 = decltype(r0)::value, QQ = decltype(qq)::value;
      const PolyLaunch g = polybank_geometry(c, 1, F);
      return polybank_launch(c, "synthesizer", synthesizer_real_os_kernel<R0, QQ>, g, st, u, ldu, x, c->d_tab, c->d_tw, c->d_tw2, c->T, c->lgT, c->FP,
                             F, g.per, (const cpx *) c->hist[c->cur], (cpx *) c->hist[c->cur ^ 1], rows_aligned(u, ldu), stream_aligned(x),
                             c->OS == 2 ? 1 : 2, c->phase);
    });
  });
  return rc == POLYBANK_UNSERVED ? set_err(TSDGPU_ERR_UNSUPPORTED, "synthesizer_step: %d taps per hop sample at oversampling %d", c->P, c->OS) : rc;
}

}  // namespace tsdgpu
