// synthesizer.hip -- maximally decimated polyphase synthesis bank: M channel rows into ONE wideband complex stream, the dual
// of channelizer.hip.
//
//   x[p] = sum_{c < M} exp(+2 pi i c p / M) sum_m u_c[m] f[p - m M]
// computed in the fast form: with P = ceil(K / M), f zero-padded to P M and p = q M + s,
//   w_.[m] = IDFT_M(u_.[m])  (inverse, unscaled),      x[q M + s] = sum_{j < P} f[j M + s] w_s[q - j].
// A step of F frames reads F samples from each of the M rows u + c ldu and writes n = F M samples of x.
//
// One persistent kernel, channelizer_kernel end for end: a workgroup of NT = 512 threads owns R = NT / M sub-runs of 16-frame
// units (at M = 1024 one sub-run, a thread owning the positions s and s + 512); the LDS image is the channelizer's.  Shared with
// the analysis kernels: polybank_tile.hpp (device) and polybank_host.hpp (the handle's host side).
//  - load: channel-major; a (channel, sub-run) pair gives its 16 frames as one 128-B segment, 8 lanes x 16 B (2 x 8 B where the
//    rows are not 16-B aligned), written frame-major into the image with re and im swapped.
//  - transform: the frame's M points by s16::transform (M = 16 .. 1024), s16::dft8 (M = 8): forward on swapped values, which is
//    the inverse transform with re and im swapped, undone where the back end reads.
//  - back end: thread (r, s) reads w_s of the unit's 16 frames in two halves of 8, keeps the position's last P - 1 values in
//    registers and forms x[f M + s] = fma chain j = P-1 .. 0 (oldest frame first), the same chain for every frame; a wave
//    writes 512 contiguous bytes per store from M = 64.
// The P - 1 halo frames are loaded and transformed only where a sub-run starts (one unit more per sub-run, nothing stored): from
// the handle's history when they lie before the step.  The last workgroup writes the new history (the last P - 1 input frames of
// old history ++ u, per channel) into the other buffer.
// The oversampled bank (hop D = M / OS, OS in {2, 4}) is the sibling kernel of synthesizer_os.hip; the handle and the entry points
// below serve both.  And the real-output banks (synthesizer_real.hip: M / 2 + 1 rows into a float32 stream; synthesizer_real_os.hip: the
// same at hop D): x counts floats there.  The C entry points of all four synthesis families are at the end of this file; the other
// three files hold a kernel and its launch.
#include "common.hpp"
#include "bank_internal.hpp"
#include "polybank_host.hpp"
#include "polybank_tile.hpp"

namespace tsdgpu {
namespace {

// R0, NPOS, PP: as channelizer_kernel's.
template <int R0, int NPOS, int PP>
__global__ __launch_bounds__(CHAN_NT) void synthesizer_kernel(const cpx *__restrict__ u, int64_t ldu, cpx *__restrict__ x,
                                                             const float *__restrict__ ft, const cpx *__restrict__ TW, int M, int lgM,
                                                             int FP, int64_t F, int64_t per, const cpx *__restrict__ oh,
                                                             cpx *__restrict__ nh, int al)
{
  extern __shared__ __attribute__((aligned(16))) char syn_raw[];
  cpx *img = reinterpret_cast<cpx *>(syn_raw);
  constexpr int NT = CHAN_NT;
  constexpr int PW = PP - 1, PWA = PW > 0 ? PW : 1;      // the window: the last PW transformed frames of the position
  const int t = threadIdx.x;

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
  float g[NPOS][PP];
  cpx prev[NPOS][PWA];
#pragma unroll
  for (int a = 0; a < NPOS; a++) {
#pragma unroll
    for (int p = 0; p < PP; p++) g[a][p] = ft[p * M + s + a * NT];
#pragma unroll
    for (int k = 0; k < PWA; k++) prev[a][k] = make_float2(0.f, 0.f);
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
          cpx *dst = x + f0 * M + s + a * NT;
          // x[(f0 + i) M + s] = sum_j g[j] frame(i - j), oldest frame first
#pragma unroll
          for (int i = 0; i < 8; i++) {
            const cpx v = window_chain<PP, 1>(g[a], prev[a], cur, i);
            if (f0 + i < F) dst[(int64_t) i * M] = v;
          }
        }
        window_shift<PW>(prev[a], cur);
      }
    __syncthreads();
  }
}

int syn_launch(tsdgpu_synthesizer *c, const cpx *u, int64_t ldu, cpx *x, int64_t F, hipStream_t st)
{
  const int rc = polybank_radix(c->T, [&](auto r0, auto npos) {
    return polybank_taps(c->P, [&](auto pp) {
      constexpr int R0 = decltype(r0)::value, NPOS = decltype(npos)::value, PP = decltype(pp)::value;
      const PolyLaunch g = polybank_geometry(c, NPOS, F);
      return polybank_launch(c, "synthesizer", synthesizer_kernel<R0, NPOS, PP>, g, st, u, ldu, x, c->d_tab, c->d_tw, c->M, c->lgM, c->FP, F,
                             g.per, (const cpx *) c->hist[c->cur], (cpx *) c->hist[c->cur ^ 1], rows_aligned(u, ldu));
    });
  });
  return rc == POLYBANK_UNSERVED ? set_err(TSDGPU_ERR_UNSUPPORTED, "synthesizer_step: %d taps per channel", c->P) : rc;
}

// the create entries below: (who, synthesis, real, min_M, only_os1, per_channel, at_one)
const PolySpec SYN_CREATE = {"synthesizer_create", true, false, CHAN_MIN_M, nullptr, true, nullptr};
const PolySpec SYN_CREATE_REAL = {"synthesizer_create_real", true, true, CHAN_REAL_MIN_M,
                                  "this entry serves 1 only (2 and 4: synthesizer_create_real_oversampled)", true, nullptr};
const PolySpec SYN_CREATE_REAL_OS = {"synthesizer_create_real_oversampled", true, true, CHAN_REAL_MIN_M, nullptr, false, &SYN_CREATE_REAL};

}  // namespace
}  // namespace tsdgpu

using namespace tsdgpu;

extern "C" {

int tsdgpu_synthesizer_create(tsdgpu_synthesizer **out, int channels, const float *taps_host, int ntaps)
{
  return polybank_create(out, SYN_CREATE, channels, 1, taps_host, ntaps);
}

int tsdgpu_synthesizer_create_oversampled(tsdgpu_synthesizer **out, int channels, int oversample, const float *taps_host, int ntaps)
{
  return polybank_create(out, SYN_CREATE, channels, oversample, taps_host, ntaps);
}

int tsdgpu_synthesizer_create_real(tsdgpu_synthesizer **out, int channels, int oversample, const float *taps_host, int ntaps)
{
  return polybank_create(out, SYN_CREATE_REAL, channels, oversample, taps_host, ntaps);
}

int tsdgpu_synthesizer_create_real_oversampled(tsdgpu_synthesizer **out, int channels, int oversample, const float *taps_host, int ntaps)
{
  return polybank_create(out, SYN_CREATE_REAL_OS, channels, oversample, taps_host, ntaps);
}

int64_t tsdgpu_synthesizer_out_count(const tsdgpu_synthesizer *c, int64_t frames) { return (!c || frames < 0) ? -1 : frames * c->D; }

int tsdgpu_synthesizer_step(tsdgpu_synthesizer *c, const void *u, int64_t ldu, int64_t frames, void *x, int64_t x_capacity, int64_t *n_out,
                            void *stream)
{
  TSD_CHECK(c != nullptr, "synthesizer_step: NULL handle");
  TSD_CHECK(frames >= 0, "synthesizer_step: negative frame count");
  if (n_out) *n_out = 0;
  if (frames == 0) return TSDGPU_OK;
  const int64_t F = frames, n = F * c->D;
  TSD_CHECK(u != nullptr && x != nullptr, "synthesizer_step: NULL buffer");
  TSD_CHECK(n <= x_capacity, "synthesizer_step: the output needs %lld samples, x_capacity is %lld", (long long) n, (long long) x_capacity);
  TSD_CHECK(ldu >= F, "synthesizer_step: ldu = %lld below the %lld inputs of a channel", (long long) ldu, (long long) F);
  const size_t sz = sizeof(cpx), szx = c->real ? sizeof(float) : sizeof(cpx);
  const int rows = polybank_rows(c);
  TSD_CHECK(!ranges_overlap(x, (size_t) n * szx, u, ((size_t) (rows - 1) * (size_t) ldu + (size_t) F) * sz),
            "synthesizer_step: u and x overlap (there is no in-place form: the layouts differ)");
  hipStream_t st = (hipStream_t) stream;
  const void *du;
  void *dx = nullptr;
  int64_t dldu = F;
  bool staged = false;
  int rc;
  if ((rc = bank_stage_in(u, ldu, F, rows, sz, false, F, c->in_stage, st, &du, &dldu))) return rc;
  if ((rc = stage_out(x, (size_t) n * szx, c->out_stage, &dx, &staged))) return rc;
  if (c->real && c->OS > 1) rc = syn_real_os_launch(c, (const cpx *) du, dldu, (float *) dx, F, st);
  else if (c->real) rc = syn_real_launch(c, (const cpx *) du, dldu, (float *) dx, F, st);
  else if (c->OS > 1) rc = syn_os_launch(c, (const cpx *) du, dldu, (cpx *) dx, F, st);
  else rc = syn_launch(c, (const cpx *) du, dldu, (cpx *) dx, F, st);
  if (rc) return rc;
  if (c->HW) c->cur ^= 1;
  c->phase = (int) ((c->phase + F) % c->OS);
  if (n_out) *n_out = n;
  return finish_out(x, (size_t) n * szx, dx, staged, st);
}

int tsdgpu_synthesizer_reset(tsdgpu_synthesizer *c) { return polybank_reset(c, "synthesizer"); }

int tsdgpu_synthesizer_history_len(const tsdgpu_synthesizer *c) { return polybank_history_len(c); }

int tsdgpu_synthesizer_hop(const tsdgpu_synthesizer *c) { return polybank_hop(c); }

int tsdgpu_synthesizer_rows(const tsdgpu_synthesizer *c) { return polybank_rows_of(c); }

int tsdgpu_synthesizer_is_real(const tsdgpu_synthesizer *c) { return polybank_is_real(c); }

int tsdgpu_synthesizer_get_phase(const tsdgpu_synthesizer *c) { return polybank_get_phase(c); }

int tsdgpu_synthesizer_set_phase(tsdgpu_synthesizer *c, int64_t hops) { return polybank_set_phase(c, "synthesizer", hops); }

int tsdgpu_synthesizer_get_state(tsdgpu_synthesizer *c, void *hist_dst, void *stream)
{
  return polybank_copy_state(c, "synthesizer_get_state", hist_dst, nullptr, (hipStream_t) stream);
}

int tsdgpu_synthesizer_set_state(tsdgpu_synthesizer *c, const void *hist_src, void *stream)
{
  return polybank_copy_state(c, "synthesizer_set_state", nullptr, hist_src, (hipStream_t) stream);
}

int tsdgpu_synthesizer_destroy(tsdgpu_synthesizer *c) { return polybank_destroy(c); }

}  // extern "C"
