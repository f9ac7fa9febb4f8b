// synthesizer_os.hip -- the oversampled polyphase synthesis bank: M channel rows at hop D = M / OS, OS in {2, 4}, into ONE
// wideband complex stream; the dual of channelizer_os.hip.
//
//   x[p] = sum_{c < M} exp(+2 pi i c p / M) sum_m u_c[m] f[p - m D],   p counted over the whole stream
// in the fast form: Q = ceil(K / D), f zero-padded to Q D, w_.[m] = IDFT_M(u_.[m]) (inverse, unscaled) and p = q D + s', s' < D:
//   x[q D + s'] = sum_{j < Q} f[j D + s'] w_r[q - j],   r = (q D + s') mod M: the same position r in all Q frames.
// A step of F frames reads F samples from each of the M rows u + c ldu and writes n = F D samples of x.
//
// The sibling of synthesizer_kernel (synthesizer.hip), which stays what it is: the same 512-thread workgroup, 16-frame units,
// R = 512 / M sub-runs, LDS image and pitch, channel-major load with re and im swapped, transform, and halo unit where a sub-run
// starts -- the input side of a tile does not know the bank is oversampled.  What differs is the back end:
//  - thread (rr, r) still owns position r of the transformed frames and keeps the position's last Q - 1 values in registers, but
//    its taps are g[j] = f[j D + (r mod D)] and it has an output only at every OS-th hop: those with (phase + q) mod OS =
//    floor(r / D), phase = the hops the stream consumed before the step, modulo OS.  The output is the chain j = Q-1 .. 0 (oldest
//    frame first) and lands at x[q D + (r mod D)].
//  - a half unit starts at a multiple of 8 frames and OS divides 8: frame i of a half is owned where (i mod OS) = (floor(r / D) -
//    phase) mod OS, the same test in every half, no register indexed at run time.  From D = 64 the test is wave-uniform and a
//    wave skips the chains it does not own (1 / OS of the multiply-adds of synthesizer_kernel at P = Q); below, lanes diverge.
//  - a hop's D outputs are the threads floor(r / D) = (phase + q) mod OS of the sub-run: D contiguous samples, 512 B from D = 64.
// OS is a launch argument, not a template parameter: the instantiations are those of synthesizer_kernel, <R0, NPOS, Q>.
// The last workgroup writes the new history (the last Q - 1 input frames of old history ++ u, per channel) into the other buffer.
// The entry points are synthesizer.hip's; this file is the kernel and its launch.
#include "polybank_host.hpp"
#include "polybank_tile.hpp"

namespace tsdgpu {
namespace {

// R0, NPOS as synthesizer_kernel's; QQ = Q taps per hop sample; lgOS = 1, 2; phase < OS.
template <int R0, int NPOS, int QQ>
__global__ __launch_bounds__(CHAN_NT) void synthesizer_os_kernel(const cpx *__restrict__ u, int64_t ldu, cpx *__restrict__ x,
                                                                const float *__restrict__ ft, const cpx *__restrict__ TW, int M, int lgM,
                                                                int FP, int64_t F, int64_t per, const cpx *__restrict__ oh,
                                                                cpx *__restrict__ nh, int al, int lgOS, int phase)
{
  extern __shared__ __attribute__((aligned(16))) char syn_os_raw[];
  cpx *img = reinterpret_cast<cpx *>(syn_os_raw);
  constexpr int NT = CHAN_NT;
  constexpr int PW = QQ - 1, PWA = PW > 0 ? PW : 1;      // the window: the last PW transformed frames of the position
  const int t = threadIdx.x;
  const int lgD = lgM - lgOS, D = 1 << lgD, OSM = (1 << lgOS) - 1;

  // input frame f of channel c: history before 0 (zeros before that); frames from F on are zeros and never reach a stored output
  auto fetch = [&](int c, int64_t f) -> cpx {
    if (f < 0) return PW > 0 && f >= -PW ? oh[c * PW + PW + (int) f] : make_float2(0.f, 0.f);
    return f < F ? u[(int64_t) c * ldu + f] : make_float2(0.f, 0.f);
  };

  // the new history: per channel the last PW frames of (old history ++ u[c][0, F))
  if (blockIdx.x == gridDim.x - 1)
    for (int i = t; i < PW * M; i += NT) {
      const int c = i / PWA, k = i - c * PWA;
      nh[i] = fetch(c, F - PW + k);
    }

  const SubRun sr = sub_run<NPOS>(t, M, lgM, per);
  const int s = sr.s, r = sr.r;
  float g[NPOS][QQ];
  cpx prev[NPOS][PWA];
  int sel[NPOS];                                         // frame i of a half unit is the position's where (i mod OS) == sel
#pragma unroll
  for (int a = 0; a < NPOS; a++) {
#pragma unroll
    for (int p = 0; p < QQ; p++) g[a][p] = ft[p * M + s + a * NT];
#pragma unroll
    for (int k = 0; k < PWA; k++) prev[a][k] = make_float2(0.f, 0.f);
    sel[a] = (((s + a * NT) >> lgD) - phase) & OSM;
  }

  const int tpt = R0 ? M >> 4 : 1;
  // it = -1: the unit before the sub-run, for its last PW transformed frames only
  for (int64_t it = PW > 0 ? -1 : 0; it < per; it++) {
    // channel-major load: item (k, c, rr) = frames 2k, 2k + 1 of sub-run rr's unit, channel c; 8 lanes per 128-B segment
#pragma unroll 4
    for (int v = 0; v < 8 * NPOS; v++) {
      const TileItem q = tile_item(t + NT * v, M, lgM, sr.R, per, it);
      const int k = q.k, c = q.c, rr = q.rr;
      const int64_t f = q.f;
      cpx a, b;
      if (al && f >= 0 && f + 1 < F) {
        const float4 q = *reinterpret_cast<const float4 *>(u + (int64_t) c * ldu + f);
        a = make_float2(q.x, q.y);
        b = make_float2(q.z, q.w);
      } else {
        a = fetch(c, f);
        b = fetch(c, f + 1);
      }
      cpx *dst = img + (rr * 16 + 2 * k) * FP + s16::pad(c);
      dst[0] = make_float2(a.y, a.x);
      dst[FP] = make_float2(b.y, b.x);
    }
    __syncthreads();

    // from here to the back end the tile is a tile of synthesizer_kernel: the transform is its own
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

    // back end: position s (and s + NT) of the thread's sub-run, 8 frames at a time
#pragma unroll
    for (int a = 0; a < NPOS; a++)
      for (int h = 0; h < 2; h++) {
        cpx cur[8];
        const int64_t f0 = ((sr.u0 + it) * 16) + 8 * h;
        const cpx *src = img + (r * 16 + 8 * h) * FP + s16::pad(s + a * NT);
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const cpx w = src[k * FP];
          cur[k] = make_float2(w.y, w.x);
        }
        if (it >= 0) {
          cpx *dst = x + (f0 << lgD) + ((s + a * NT) & (D - 1));
          // x[(f0 + i) D + (s mod D)] = sum_j g[j] frame(i - j), oldest frame first, at the hops the position owns
#pragma unroll
          for (int i = 0; i < 8; i++)
            if ((i & OSM) == sel[a]) {
              const cpx v = window_chain<QQ, 1>(g[a], prev[a], cur, i);
              if (f0 + i < F) dst[(int64_t) i << lgD] = v;
            }
        }
        window_shift<PW>(prev[a], cur);
      }
    __syncthreads();
  }
}

}  // namespace

int syn_os_launch(tsdgpu_synthesizer *c, const cpx *u, int64_t ldu, cpx *x, int64_t F, hipStream_t st)
{
  if (c->OS != 2 && c->OS != 4) return set_err(TSDGPU_ERR_UNSUPPORTED, "synthesizer_step: oversampling %d", c->OS);
  const int rc = polybank_radix(c->T, [&](auto r0, auto npos) {
    return polybank_taps(c->P, [&](auto qq) {
      constexpr int R0 = decltype(r0)::value, NPOS = decltype(npos)::value, QQ = decltype(qq)::value;
      const PolyLaunch g = polybank_geometry(c, NPOS, F);
      return polybank_launch(c, "synthesizer", synthesizer_os_kernel<R0, NPOS, QQ>, g, st, u, ldu, x, c->d_tab, c->d_tw, c->M, c->lgM, c->FP, F,
                             g.per, (const cpx *) c->hist[c->cur], (cpx *) c->hist[c->cur ^ 1], rows_aligned(u, ldu), c->OS == 2 ? 1 : 2,
                             c->phase);
    });
  });
  return rc == POLYBANK_UNSERVED ? set_err(TSDGPU_ERR_UNSUPPORTED, "synthesizer_step: %d taps per hop sample at oversampling %d", c->P, c->OS) : rc;
}

}  // namespace tsdgpu
