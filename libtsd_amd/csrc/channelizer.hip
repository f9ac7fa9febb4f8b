// channelizer.hip -- maximally decimated polyphase analysis bank: ONE wideband complex stream into M channel rows.
//
//   y_c[m] = sum_k h[k] x[n_m - k] exp(-2 pi i c (n_m - k) / M),  n_m = m M + M - 1,  c < M
// computed in the fast form: with P = ceil(K / M), h zero-padded to P M and g_p[s] = h[p M + M - 1 - s],
//   v_s[m] = sum_{p < P} g_p[s] x[(m - p) M + s],      y_.[m] = DFT_M(v_.[m])  (forward, unscaled).
// A step of F frames (n = F M samples) writes F outputs to each of the M rows y + c ldy: the (C, n) layout the channel banks read.
//
// One persistent kernel.  A workgroup of NT = 512 threads owns R = NT / M streams of frames ("sub-runs": contiguous ranges of
// 16-frame units; at M = 1024 one sub-run, a thread owning the positions s and s + 512); per iteration every sub-run advances by
// one unit, so the workgroup's tile is 16 R frames x M channels = 8 Ki points (16 Ki at M = 1024), one LDS image of 68-74 KiB
// (137 KiB at M = 1024): two workgroups per CU where the registers allow it, one loading while one transforms.
//  - front: thread (r, s) owns position s of sub-run r.  It loads the unit's samples x[f M + s] in two halves of 8 frames (8
//    loads in flight; a wave reads 512 contiguous bytes per load from M = 64) and keeps the position's last P - 1 samples in
//    registers -- the P - 1 halo frames are read from memory only where a sub-run starts: from the handle's history when they lie
//    before the step -- and forms v_s[f] = fma chain p = P-1 .. 0 (oldest sample first), the same chain for every frame.
//  - transform: the frame's M points in registers + LDS by s16::transform (M = 16 .. 1024), s16::dft8 (M = 8).
//  - store: the bins are read back channel-major; a (channel, sub-run) pair receives its 16 frames as one 128-B segment.
// The last workgroup writes the new history (the last (P - 1) M samples of old history ++ x) into the other buffer.
// The handle also serves the oversampled bank (hop D = M / OS, OS in {2, 4}): its kernel family is channelizer_os.hip, and the
// entry points below count a step in hops of D samples; at OS = 1 they are what they were.  And the real-input bank
// (channelizer_real.hip: a float32 stream into M / 2 + 1 rows; channelizer_real_os.hip at OS > 1): n and the history count floats there.
// The C entry points of all four analysis families are at the end of this file; the other three files hold a kernel and its launch.
// Shared with all seven other bank files: polybank_tile.hpp (device; it says why the transform block is not in it) and
// polybank_host.hpp (the handle, the create path, the accessor bodies, the launch and the dispatch over M and the taps).
#include "common.hpp"
#include "bank_internal.hpp"
#include "polybank_host.hpp"
#include "polybank_tile.hpp"

namespace tsdgpu {
namespace {

// R0 in {16, 8, 4, 2}: M = R0 16^a >= 16 through s16::transform; R0 = 0: M = 8 through s16::dft8.
// NPOS positions per thread: 1; 2 at M = 1024 (positions s and s + 512, the transforms in two rounds of 8 frames).
// PP = P, the taps of a polyphase branch: the window and the fma chains are straight-line code in registers.
template <int R0, int NPOS, int PP>
__global__ __launch_bounds__(CHAN_NT) void channelizer_kernel(const cpx *__restrict__ x, cpx *__restrict__ y, int64_t ldy,
                                                              const float *__restrict__ gt, const cpx *__restrict__ TW, int M, int lgM,
                                                              int FP, int64_t F, int64_t per, const cpx *__restrict__ oh,
                                                              cpx *__restrict__ nh, int al)
{
  extern __shared__ __attribute__((aligned(16))) char chan_raw[];
  cpx *img = reinterpret_cast<cpx *>(chan_raw);
  constexpr int NT = CHAN_NT;
  constexpr int PW = PP - 1, PWA = PW > 0 ? PW : 1;      // the window: the last PW samples of the position
  const int t = threadIdx.x;
  const int HW = PW * M;
  const int64_t n = F * M;

  // the new history: the last HW samples of (old history ++ x[0, n))
  if (blockIdx.x == gridDim.x - 1)
    for (int i = t; i < HW; i += NT) {
      const int64_t g = n - HW + i;
      nh[i] = g < 0 ? oh[HW + g] : x[g];
    }

  const SubRun sr = sub_run<NPOS>(t, M, lgM, per);
  const int s = sr.s, r = sr.r;
  // frame f of the stream, position s: history before 0; frames from F on (the tail of the last unit, idle sub-runs) read
  // the last frame and are never stored
  auto sample = [&](int64_t f, int a) -> cpx {
    f = min(f, F - 1);
    const cpx *b = f < 0 ? oh + (f + PW) * M : x + f * M;
    return b[s + a * NT];
  };
  float g[NPOS][PP];
  cpx prev[NPOS][PWA];
#pragma unroll
  for (int a = 0; a < NPOS; a++) {
#pragma unroll
    for (int p = 0; p < PP; p++) g[a][p] = gt[p * M + s + a * NT];
#pragma unroll
    for (int k = 0; k < PW; k++) prev[a][k] = sample(sr.u0 * 16 - PW + k, a);
  }

  const int tpt = R0 ? M >> 4 : 1;
  for (int64_t it = 0; it < per; it++) {
#pragma unroll
    for (int a = 0; a < NPOS; a++)
      for (int h = 0; h < 2; h++) {
        cpx cur[8];
        const int64_t f0 = ((sr.u0 + it) << 4) + 8 * h;
#pragma unroll
        for (int k = 0; k < 8; k++) cur[k] = sample(f0 + k, a);
        cpx *dst = img + (r * 16 + 8 * h) * FP + s16::pad(s + a * NT);
        // v_s[f0 + i] = sum_p g[p] frame(i - p), oldest sample first
#pragma unroll
        for (int i = 0; i < 8; i++) dst[i * FP] = window_chain<PP, 1>(g[a], prev[a], cur, i);
        window_shift<PW>(prev[a], cur);
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

    store_rows<NPOS>(img, y, ldy, M, lgM, FP, F, per, it, sr.R, al, t);
    __syncthreads();
  }
}

int chan_launch(tsdgpu_channelizer *c, const cpx *x, cpx *y, int64_t ldy, int64_t F, hipStream_t st)
{
  const int rc = polybank_radix(c->T, [&](auto r0, auto npos) {
    return polybank_taps(c->P, [&](auto pp) {
      constexpr int R0 = decltype(r0)::value, NPOS = decltype(npos)::value, PP = decltype(pp)::value;
      const PolyLaunch g = polybank_geometry(c, NPOS, F);
      return polybank_launch(c, "channelizer", channelizer_kernel<R0, NPOS, PP>, g, st, x, y, ldy, c->d_tab, c->d_tw, c->M, c->lgM, c->FP, F,
                             g.per, (const cpx *) c->hist[c->cur], (cpx *) c->hist[c->cur ^ 1], rows_aligned(y, ldy));
    });
  });
  return rc == POLYBANK_UNSERVED ? set_err(TSDGPU_ERR_UNSUPPORTED, "channelizer_step: %d taps per channel", c->P) : rc;
}

// the create entries below: (who, synthesis, real, min_M, only_os1, per_channel, at_one)
const PolySpec CHAN_CREATE = {"channelizer_create", false, false, CHAN_MIN_M, nullptr, true, nullptr};
const PolySpec CHAN_CREATE_REAL = {"channelizer_create_real", false, true, CHAN_REAL_MIN_M,
                                   "served is 1 (tsdgpu_channelizer_create_real_oversampled serves 2 and 4)", true, nullptr};
const PolySpec CHAN_CREATE_REAL_OS = {"channelizer_create_real_oversampled", false, true, CHAN_REAL_MIN_M, nullptr, false, &CHAN_CREATE_REAL};

}  // namespace
}  // namespace tsdgpu

using namespace tsdgpu;

extern "C" {

int tsdgpu_channelizer_create(tsdgpu_channelizer **out, int channels, const float *taps_host, int ntaps)
{
  return polybank_create(out, CHAN_CREATE, channels, 1, taps_host, ntaps);
}

int tsdgpu_channelizer_create_oversampled(tsdgpu_channelizer **out, int channels, int oversample, const float *taps_host, int ntaps)
{
  return polybank_create(out, CHAN_CREATE, channels, oversample, taps_host, ntaps);
}

int tsdgpu_channelizer_create_real(tsdgpu_channelizer **out, int channels, int oversample, const float *taps_host, int ntaps)
{
  return polybank_create(out, CHAN_CREATE_REAL, channels, oversample, taps_host, ntaps);
}

int tsdgpu_channelizer_create_real_oversampled(tsdgpu_channelizer **out, int channels, int oversample, const float *taps_host, int ntaps)
{
  return polybank_create(out, CHAN_CREATE_REAL_OS, channels, oversample, taps_host, ntaps);
}

int64_t tsdgpu_channelizer_out_count(const tsdgpu_channelizer *c, int64_t n) { return (!c || n < 0) ? -1 : n / c->D; }

int tsdgpu_channelizer_step(tsdgpu_channelizer *c, const void *x, int64_t n, void *y, int64_t ldy, int64_t y_capacity, int64_t *n_out,
                            void *stream)
{
  TSD_CHECK(c != nullptr, "channelizer_step: NULL handle");
  TSD_CHECK(n >= 0, "channelizer_step: negative length");
  if (n_out) *n_out = 0;
  if (n == 0) return TSDGPU_OK;
  TSD_CHECK(n % c->D == 0, "channelizer_step: n = %lld is not a whole number of %d-sample %s", (long long) n, c->D,
            c->OS == 1 ? "frames" : "hops");
  const int64_t F = n / c->D;
  TSD_CHECK(x != nullptr && y != nullptr, "channelizer_step: NULL buffer");
  TSD_CHECK(F <= y_capacity, "channelizer_step: a channel's output needs %lld samples, y_capacity is %lld", (long long) F, (long long) y_capacity);
  TSD_CHECK(ldy >= F, "channelizer_step: ldy = %lld below the %lld outputs of a channel", (long long) ldy, (long long) F);
  const size_t sz = sizeof(cpx), szx = c->real ? sizeof(float) : sizeof(cpx);
  const int rows = polybank_rows(c);
  TSD_CHECK(!ranges_overlap(x, (size_t) n * szx, y, ((size_t) (rows - 1) * (size_t) ldy + (size_t) F) * sz),
            "channelizer_step: x and y overlap (there is no in-place form: the layouts differ)");
  hipStream_t st = (hipStream_t) stream;
  const void *dx;
  void *dy = nullptr;
  int64_t dldy = F;
  bool staged = false;
  int rc;
  if ((rc = stage_in(x, (size_t) n * szx, c->in_stage, st, &dx))) return rc;
  if ((rc = bank_stage_out(y, ldy, rows, sz, false, F, c->out_stage, &dy, &dldy, &staged))) return rc;
  if (c->real && c->OS > 1) rc = chan_real_os_launch(c, (const float *) dx, (cpx *) dy, dldy, F, st);
  else if (c->real) rc = chan_real_launch(c, (const float *) dx, (cpx *) dy, dldy, F, st);
  else if (c->OS > 1) rc = chan_os_launch(c, (const cpx *) dx, (cpx *) dy, dldy, F, st);
  else rc = chan_launch(c, (const cpx *) dx, (cpx *) dy, dldy, F, st);
  if (rc) return rc;
  if (c->HW) c->cur ^= 1;
  c->phase = (int) ((c->phase + F) % c->OS);
  if (n_out) *n_out = F;
  return bank_finish_out(y, ldy, F, rows, sz, dy, dldy, staged, st);
}

int tsdgpu_channelizer_reset(tsdgpu_channelizer *c) { return polybank_reset(c, "channelizer"); }

int tsdgpu_channelizer_history_len(const tsdgpu_channelizer *c) { return polybank_history_len(c); }

int tsdgpu_channelizer_hop(const tsdgpu_channelizer *c) { return polybank_hop(c); }

int tsdgpu_channelizer_rows(const tsdgpu_channelizer *c) { return polybank_rows_of(c); }

int tsdgpu_channelizer_is_real(const tsdgpu_channelizer *c) { return polybank_is_real(c); }

int tsdgpu_channelizer_get_phase(const tsdgpu_channelizer *c) { return polybank_get_phase(c); }

int tsdgpu_channelizer_set_phase(tsdgpu_channelizer *c, int64_t hops) { return polybank_set_phase(c, "channelizer", hops); }

int tsdgpu_channelizer_get_state(tsdgpu_channelizer *c, void *hist_dst, void *stream)
{
  return polybank_copy_state(c, "channelizer_get_state", hist_dst, nullptr, (hipStream_t) stream);
}

int tsdgpu_channelizer_set_state(tsdgpu_channelizer *c, const void *hist_src, void *stream)
{
  return polybank_copy_state(c, "channelizer_set_state", nullptr, hist_src, (hipStream_t) stream);
}

int tsdgpu_channelizer_destroy(tsdgpu_channelizer *c) { return polybank_destroy(c); }

}  // extern "C"

