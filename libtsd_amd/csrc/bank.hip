// bank.hip -- C-channel banks of the direct FIR and of the SOS cascade: many streams of ONE filter in one launch.
//
// Stands behind FiltreRIF<T,Tc>::step and ChaineSOIS<T,T,T>::step applied to every column of an n x C column-major Tab
// (libtsd core/src/filtrage/filtre-rt.cc:53-109, 303-400).  Channel c of a step reads x + c ldx and writes y + c ldy, n
// samples each; every channel carries its own state exactly as its own tsdgpu_fir / tsdgpu_sos handle would.
//
// FIR bank: the direct kernel's scheme (fir.hip) on a (tile, channel) grid.  A tile stages its inputs in LDS with 16-B loads
// wherever a whole 16-B unit lies inside the channel's block -- the first tile of a channel takes its halo from the channel's
// history row, the ragged last tile its tail from zeros, each element by element only in the one or two units that straddle
// an edge -- and stores its outputs back through LDS in 16-B units, the channel's last partial unit element by element.
// (fir_direct_kernel keeps 16-B accesses for interior tiles only: at n = 4096 every one of its tiles is an edge tile.)
// The multiply-adds are the direct kernel's, in its order: a channel's output is bit-identical to a TSDGPU_FIR_DIRECT handle.
// The channel's last tile also writes the channel's new history: one launch per step.
// Created with TSDGPU_FIR_OVERLAP_SAVE or TSDGPU_FIR_AUTO the bank also owns the 1024-point overlap-save plan (ols_bank.hip) and
// chooses between the two schemes per step; both read and write the same C x HL history rows.
//
// SOS bank: sos_kernel's block-parallel cascade (sos.hip) with a channel grid dimension.  Each channel has its own state slot
// (the single-stream record layout: seeded flag, then the memories), and the wave that owns a channel's last chunk also runs
// its ragged end (sos_tail_kernel's two stages): one launch per step.  With enough channels to fill the chip every channel is
// ONE chunk (exact state, no warm-up); few channels with long blocks are cut into chunks with warm-ups like a single stream.
// Blocks of 2^20 samples and more go channel by channel through tsdgpu_sos_step on the channel's slot.
#include "common.hpp"
#include "fir_internal.hpp"
#include "sos_internal.hpp"
#include "bank_internal.hpp"
#include <algorithm>

struct tsdgpu_fir_bank {
  // a direct handle: reversed padded taps (d_hrev), KP; its own history serves no channel.  With the overlap-save scheme it also
  // carries the 1024-point plan's tables (d_H, ols_L: ols_bank.hip)
  tsdgpu_fir *proto = nullptr;
  int64_t C = 0;
  int method = TSDGPU_FIR_DIRECT;       // as requested at creation
  bool ols = false;                     // the overlap-save plan exists (2 <= K <= 961 and the method asks for it)
  int ols_grid = 0;                     // its persistent grid (resident waves)
  int last = TSDGPU_FIR_DIRECT;         // the scheme of the last step
  bool stepped = false;
  int HL = 0;                           // samples per history row: both schemes read the row's END, so the longer need serves both
  void *hist[2] = {nullptr, nullptr};   // C rows of HL samples each (double-buffered), newest last
  int cur = 0;
  int ymax = 0;                  // the grid's y limit (channels per launch)
  tsdgpu::DevBuf in_stage, out_stage;
};

struct tsdgpu_sos_bank {
  tsdgpu_sos *proto = nullptr;   // the section tables, gain, halo; its own state slots serve no channel
  int64_t C = 0;
  float *st[2] = {nullptr, nullptr};    // C state records of STATE_FLOATS floats each (double-buffered)
  int cur = 0;
  int ymax = 0;
  tsdgpu::DevBuf in_stage, out_stage;
};

namespace tsdgpu {
namespace {

// The common checks of a step (n, pointers, strides, overlap)
int bank_step_checks(const char *who, const void *x, int64_t ldx, const void *y, int64_t ldy, int64_t n, int64_t C, size_t sz)
{
  TSD_CHECK(x != nullptr && y != nullptr, "%s: NULL buffer", who);
  TSD_CHECK(ldx >= n && ldy >= n, "%s: leading dimensions (ldx = %lld, ldy = %lld) below n = %lld", who, (long long) ldx,
            (long long) ldy, (long long) n);
  const size_t ex = ((size_t) (C - 1) * (size_t) ldx + (size_t) n) * sz, ey = ((size_t) (C - 1) * (size_t) ldy + (size_t) n) * sz;
  TSD_CHECK(!ranges_overlap(x, ex, y, ey) || (x == y && ldx == ldy),
            "%s: x and y overlap (in place needs x == y and ldx == ldy)", who);
  return TSDGPU_OK;
}

// ------------------------------------------------------------------ FIR bank kernel
// fir_direct_kernel's LDS image and lane windows (fir.hip), grid (tile, channel c0 + blockIdx.y).  AL: 16-B aligned output rows
// (whole output units go out as aligned 16-B stores; other rows take 16-B stores at 4-B alignment, which hipcc splits).
template <typename T, typename TC, int R, int THREADS, bool AL>
__global__ __launch_bounds__(THREADS) void fir_bank_kernel(const T *__restrict__ x, int64_t ldx, T *__restrict__ y, int64_t ldy,
                                                            const TC *__restrict__ hrev, int KP, int64_t n,
                                                            const T *__restrict__ old_hist, T *__restrict__ new_hist, int HL, int64_t c0)
{
  constexpr int TILE = THREADS * R;
  constexpr int VEC = 16 / (int) sizeof(T);          // samples per 16 B
  constexpr int P = VEC;                             // pad samples per segment
  constexpr int SP = R + P;                          // segment pitch in samples (80 B)
  static_assert(R * sizeof(T) == 64, "one lane segment is 64 bytes");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T *L = reinterpret_cast<T *>(smem_raw);

  const int64_t ch = c0 + blockIdx.y;
  x += ch * ldx;
  y += ch * ldy;
  const T *oh = old_hist + ch * HL;
  const T *hp = oh + (HL - KP);                      // the halo's source: the last KP samples of the channel's history
  const int64_t tile0 = (int64_t) blockIdx.x * TILE;
  const int H = KP;
  const int total = TILE + H;                        // samples 0 .. total-1 (sample 0 unused)

  // the channel's last tile writes its new history (the last HL samples of old history ++ x) into the other buffer
  if (blockIdx.x == gridDim.x - 1) {
    T *nh = new_hist + ch * HL;
    for (int i = threadIdx.x; i < HL; i += THREADS) {
      const int64_t g = n - HL + i;
      nh[i] = g < 0 ? oh[HL + g] : x[g];
    }
  }

  // chunk c = samples [c*VEC + 1, c*VEC + 1 + VEC) of the tile (fir_direct_kernel's interior layout): one 16-B load when the
  // unit lies inside [0, n), else element by element from the history (before 0) or zeros (from n on)
  const int nchunks = (total - 1 + VEC - 1) / VEC;
  for (int c0i = threadIdx.x; c0i < nchunks; c0i += 4 * THREADS) {
    f4u q4[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int c = c0i + u * THREADS;
      if (c < nchunks) {
        const int64_t g0 = tile0 - H + 1 + (int64_t) c * VEC;
        if (g0 >= 0 && g0 + VEC <= n) {
          q4[u] = *reinterpret_cast<const f4u *>(x + g0);
        } else {
          T *e = reinterpret_cast<T *>(&q4[u]);
#pragma unroll
          for (int k = 0; k < VEC; k++) {
            const int64_t g = g0 + k;
            e[k] = g < 0 ? hp[H + g] : g < n ? x[g] : zero_of(T{});
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int c = c0i + u * THREADS;
      if (c < nchunks) {
        const int q = c * VEC;
        *reinterpret_cast<float4 *>(L + q + (q / R) * P) = make_float4(q4[u].x, q4[u].y, q4[u].z, q4[u].w);
      }
    }
  }
  __syncthreads();

  // lane window: w[i] = sample t*R + 1 + i = Lw[(i / R) * SP + i % R], out[r] = sum_j hrev[j] * w[r + j]
  const T *Lw = L + threadIdx.x * SP;
  T acc[R], A[R], B[R];
  auto load_seg = [&](T (&dst)[R], const T *seg) {
#pragma unroll
    for (int v4 = 0; v4 < R / VEC; v4++) {
      const float4 q4 = *reinterpret_cast<const float4 *>(seg + v4 * VEC);
      const T *e = reinterpret_cast<const T *>(&q4);
#pragma unroll
      for (int k = 0; k < VEC; k++) dst[v4 * VEC + k] = e[k];
    }
  };
#pragma unroll
  for (int r = 0; r < R; r++) acc[r] = zero_of(T{});
  if (tile0 + (int64_t) threadIdx.x * R < n) {       // (lanes wholly past the channel's end have nothing to compute)
    load_seg(A, Lw);
    const int nchunk = KP / R;  // even by construction
#pragma unroll 2
    for (int c = 0; c < nchunk; c += 2) {
      const TC *h0 = hrev + c * R;
      load_seg(B, Lw + (c + 1) * SP);
#pragma unroll
      for (int jj = 0; jj < R; jj++) {
        const TC hv = h0[jj];
#pragma unroll
        for (int r = 0; r < R; r++) {
          const int idx = r + jj;
          acc[r] = mac(acc[r], idx < R ? A[idx] : B[idx - R], hv);
        }
      }
      // the last refill reads past the lane's window; the staging area is over-allocated by two segments
      load_seg(A, Lw + (c + 2) * SP);
#pragma unroll
      for (int jj = 0; jj < R; jj++) {
        const TC hv = h0[R + jj];
#pragma unroll
        for (int r = 0; r < R; r++) {
          const int idx = r + jj;
          acc[r] = mac(acc[r], idx < R ? B[idx] : A[idx - R], hv);
        }
      }
    }
  }

  // outputs go back through LDS: coalesced 16-B stores of whole units, the channel's last partial unit element by element
  __syncthreads();
  T *Lo = L + threadIdx.x * SP;
#pragma unroll
  for (int v4 = 0; v4 < R / VEC; v4++) {
    float4 q4;
    T *e = reinterpret_cast<T *>(&q4);
#pragma unroll
    for (int k = 0; k < VEC; k++) e[k] = acc[v4 * VEC + k];
    *reinterpret_cast<float4 *>(Lo + v4 * VEC) = q4;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < TILE / VEC; c += THREADS) {
    const int64_t o = tile0 + (int64_t) c * VEC;
    if (o >= n) break;
    const float4 q4 = *reinterpret_cast<const float4 *>(L + (c / (R / VEC)) * SP + (c % (R / VEC)) * VEC);
    if (o + VEC <= n) {
      if (AL) *reinterpret_cast<float4 *>(y + o) = q4;
      else *reinterpret_cast<f4u *>(y + o) = f4u{q4.x, q4.y, q4.z, q4.w};
    } else {
      const T *e = reinterpret_cast<const T *>(&q4);
      for (int k = 0; k < VEC && o + k < n; k++) y[o + k] = e[k];
    }
  }
}

template <typename T, typename TC, int R>
int fir_bank_launch(tsdgpu_fir_bank *b, const void *x, int64_t ldx, void *y, int64_t ldy, int64_t n, hipStream_t st)
{
  constexpr int THREADS = 256;
  constexpr int TILE = THREADS * R;
  const tsdgpu_fir *f = b->proto;
  const int KP = f->KP;
  const size_t lds = ((size_t) (TILE + KP) / R + 3) * 80;       // fir.hip: launch_direct
  const int64_t tiles = cdiv(n, TILE);
  if (tiles * THREADS > 0x7fffffff) return set_err(TSDGPU_ERR_UNSUPPORTED, "fir_bank_step: n = %lld too large for one launch", (long long) n);
  const T *oldh = (const T *) b->hist[b->cur];
  T *newh = (T *) b->hist[b->cur ^ 1];
  const bool al = ((uintptr_t) y & 15) == 0 && (ldy * (int64_t) sizeof(T)) % 16 == 0;
  for (int64_t c0 = 0; c0 < b->C; c0 += b->ymax) {
    const unsigned cy = (unsigned) std::min<int64_t>(b->ymax, b->C - c0);
    if (al)
      hipLaunchKernelGGL((fir_bank_kernel<T, TC, R, THREADS, true>), dim3((unsigned) tiles, cy), dim3(THREADS), lds, st, (const T *) x, ldx,
                         (T *) y, ldy, (const TC *) f->d_hrev, KP, n, oldh, newh, b->HL, c0);
    else
      hipLaunchKernelGGL((fir_bank_kernel<T, TC, R, THREADS, false>), dim3((unsigned) tiles, cy), dim3(THREADS), lds, st, (const T *) x, ldx,
                         (T *) y, ldy, (const TC *) f->d_hrev, KP, n, oldh, newh, b->HL, c0);
    TSD_HIP(hipGetLastError());
  }
  return TSDGPU_OK;
}

// ------------------------------------------------------------------ SOS bank kernel
// sos_kernel<NCH, 0> (sos.hip) with grid (chunk, channel c0 + blockIdx.y), ld in floats; the wave of a channel's last chunk
// goes on with the channel's ragged end (sos_tail_kernel) and publishes the channel's state.  x, y: 16-B aligned rows.
template <int NCH>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SOS_WPE, SOS_WPE))) void sos_bank_kernel(
    const float *__restrict__ x, int64_t ldx, float *__restrict__ y, int64_t ldy, const SosSection *__restrict__ sec, int nsec,
    float gain, const float *__restrict__ st_in, float *__restrict__ st_out, int64_t nfl, int spc, int warm_sub, int warm_nar,
    int64_t c0)
{
  __shared__ __attribute__((aligned(16))) float lds[64 * LDS_LANE_PITCH];
  __shared__ float sst[SOS_MAX_SEC * 8];          // running state per (section, channel): 4 floats
  __shared__ float buf[LANE_FLOATS];
  const int lane = threadIdx.x;
  const int64_t ch = c0 + blockIdx.y;
  x += ch * ldx;
  y += ch * ldy;
  st_in += ch * STATE_FLOATS;
  st_out += ch * STATE_FLOATS;
  const int64_t n_sub = nfl / SUB_FLOATS;
  const int64_t chunk = blockIdx.x;
  const int64_t t_first = chunk * spc;
  const int64_t t_last = min(t_first + spc, n_sub);
  const bool first_chunk = chunk == 0;
  const bool seeded = st_in[0] != 0.f;

  if (first_chunk) state_load(sst, st_in, sec, nsec, lane);
  else
    for (int i = lane; i < nsec * 8; i += 64) sst[i] = 0.f;
  wave_sync();

  int64_t t = t_first;
  if (!first_chunk) {
    t = t_first - warm_sub;
    const float *xw = x + t * SUB_FLOATS - (int64_t) warm_nar * (64 * NARROW_FLOATS);
    for (int w = 0; w < warm_nar; w++) {
      const float4 q = *reinterpret_cast<const float4 *>(xw + (int64_t) w * (64 * NARROW_FLOATS) + 4 * lane);
      float v4[NARROW_FLOATS] = {q.x, q.y, q.z, q.w};
      sos_cascade<NCH, NARROW_FLOATS, true>(v4, sec, nsec, sst, lane, false);
    }
  }

  for (; t < t_last; t++) {
    const float *xt = x + t * SUB_FLOATS;
    float v[LANE_FLOATS];
#pragma unroll
    for (int i = 0; i < LANE_QUADS; i++) {
      const int p = 4 * (i * 64 + lane);
      const float4 q = *reinterpret_cast<const float4 *>(xt + p);
      *reinterpret_cast<float4 *>(&lds[sos_img(p)]) = q;
    }
    wave_sync();
#pragma unroll
    for (int i = 0; i < LANE_QUADS; i++) {
      const float4 q = *reinterpret_cast<const float4 *>(&lds[sos_img(lane * LANE_FLOATS + 4 * i)]);
      v[4 * i] = q.x; v[4 * i + 1] = q.y; v[4 * i + 2] = q.z; v[4 * i + 3] = q.w;
    }
    wave_sync();

    sos_cascade<NCH, LANE_FLOATS, false>(v, sec, nsec, sst, lane, first_chunk && !seeded && t == 0);

    if (t >= t_first) {
#pragma unroll
      for (int i = 0; i < LANE_QUADS; i++) {
        const float4 q = make_float4(v[4 * i] * gain, v[4 * i + 1] * gain, v[4 * i + 2] * gain, v[4 * i + 3] * gain);
        *reinterpret_cast<float4 *>(&lds[sos_img(lane * LANE_FLOATS + 4 * i)]) = q;
      }
      wave_sync();
      float *yt = y + t * SUB_FLOATS;
#pragma unroll
      for (int i = 0; i < LANE_QUADS; i++) {
        const int p = 4 * (i * 64 + lane);
        *reinterpret_cast<float4 *>(yt + p) = *reinterpret_cast<const float4 *>(&lds[sos_img(p)]);
      }
      wave_sync();
    }
  }
  if (blockIdx.x + 1 != gridDim.x) return;

  // ---- the channel's ragged end, floats [f0, nfl): sos_tail_kernel's two stages on the state in sst
  const int64_t f0 = n_sub * SUB_FLOATS;
  int64_t f = f0;
  const int nl = (int) ((nfl - f0) / LANE_FLOATS);
  if (nl > 0) {
    const int nf = nl * LANE_FLOATS;
    float v[LANE_FLOATS];
#pragma unroll
    for (int i = 0; i < LANE_QUADS; i++) {
      const int p = 4 * (i * 64 + lane);
      const float4 q = p < nf ? *reinterpret_cast<const float4 *>(x + f + p) : make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4 *>(&lds[(p / LANE_FLOATS) * LDS_LANE_PITCH + (p % LANE_FLOATS)]) = q;
    }
    wave_sync();
#pragma unroll
    for (int i = 0; i < LANE_QUADS; i++) {
      const float4 q = *reinterpret_cast<const float4 *>(&lds[lane * LDS_LANE_PITCH + 4 * i]);
      v[4 * i] = q.x; v[4 * i + 1] = q.y; v[4 * i + 2] = q.z; v[4 * i + 3] = q.w;
    }
    wave_sync();
    sos_cascade<NCH, LANE_FLOATS, false>(v, sec, nsec, sst, lane, !seeded && f == 0, nl - 1);
#pragma unroll
    for (int i = 0; i < LANE_QUADS; i++)
      *reinterpret_cast<float4 *>(&lds[lane * LDS_LANE_PITCH + 4 * i]) =
          make_float4(v[4 * i] * gain, v[4 * i + 1] * gain, v[4 * i + 2] * gain, v[4 * i + 3] * gain);
    wave_sync();
#pragma unroll
    for (int i = 0; i < LANE_QUADS; i++) {
      const int p = 4 * (i * 64 + lane);
      if (p < nf) *reinterpret_cast<float4 *>(y + f + p) = *reinterpret_cast<const float4 *>(&lds[(p / LANE_FLOATS) * LDS_LANE_PITCH + (p % LANE_FLOATS)]);
    }
    wave_sync();
    f += nf;
  }
  const int m = (int) (nfl - f), ms = m / NCH;
  if (ms > 0) {
    for (int i = lane; i < m; i += 64) buf[i] = x[f + i];
    wave_sync();
    const int sidx = lane / NCH, c = lane - sidx * NCH;
    const bool actif = sidx < nsec;
    const SosSection &k = sec[actif ? sidx : 0];
    const float b0 = k.b0, b1 = k.b1, b2 = k.b2, a1 = k.a1, a2 = k.a2;
    const bool df1 = k.df1 != 0.f, graine = k.seed != 0.f && !seeded && f == 0;    // first sample of the channel: seeded sections
    float *ss = &sst[(sidx * 2 + c) * 4];
    float d1 = 0.f, d2 = 0.f, x1 = 0.f, x2 = 0.f, out = 0.f;
    if (actif) { d1 = ss[0]; d2 = k.sg * (ss[0] - ss[1]); x1 = ss[2]; x2 = ss[3]; }
    for (int tt = 0; tt < ms + nsec - 1; tt++) {
      const float amont = __shfl_up(out, NCH);
      const int i = tt - sidx;
      if (actif && i >= 0 && i < ms) {
        const float xin = sidx == 0 ? buf[i * NCH + c] : amont;
        if (i == 0 && graine) d1 = d2 = x1 = x2 = xin;     // filtre-rt.cc:361-365
        float o;
        if (!df1) {
          const float d = fmaf(-a2, d2, fmaf(-a1, d1, xin));
          o = fmaf(b2, d2, fmaf(b1, d1, b0 * d));
          d2 = d1;
          d1 = d;
        } else {
          o = fmaf(-a2, d2, fmaf(-a1, d1, fmaf(b2, x2, fmaf(b1, x1, b0 * xin))));
          x2 = x1;
          x1 = xin;
          d2 = d1;
          d1 = o;
        }
        out = o;
        if (sidx == nsec - 1) buf[i * NCH + c] = o * gain;
      }
    }
    wave_sync();
    for (int i = lane; i < m; i += 64) y[f + i] = buf[i];
    if (actif) { ss[0] = d1; ss[1] = d1 - k.sg * d2; ss[2] = x1; ss[3] = x2; }
    wave_sync();
  }
  state_store(st_out, sst, sec, nsec, lane);
}

constexpr int64_t SOS_BANK_WAVES = 2048;                  // waves that fill the chip (the single-stream planner's threshold)
constexpr int64_t SOS_BANK_SINGLE_MIN = (int64_t) 1 << 20;  // blocks from this length on go through the single-stream step

int sos_bank_launch(tsdgpu_sos_bank *b, const float *x, int64_t ldx_f, float *y, int64_t ldy_f, int64_t n, hipStream_t st)
{
  const tsdgpu_sos *s = b->proto;
  const int nch = s->nch;
  const int64_t nfl = n * nch, n_sub = nfl / SUB_FLOATS;
  // one chunk per channel when the channels alone fill the chip (or the filter does not decay); else chunks with warm-ups,
  // as many as fill the chip, each at least one warm-up longer than the warm-up (sos.hip: tsdgpu_sos_step)
  int64_t spc = std::max<int64_t>(n_sub, 1), warm_sub = 0, warm_nar = 0;
  if (b->C < SOS_BANK_WAVES && n_sub > 1 && s->halo >= 0) {
    const int64_t sub_samples = SUB_FLOATS / nch, nar_samples = 64 * NARROW_FLOATS / nch;
    warm_sub = s->halo / sub_samples;
    warm_nar = cdiv(s->halo - warm_sub * sub_samples, nar_samples);
    if (warm_nar * nar_samples >= sub_samples) { warm_sub++; warm_nar = 0; }
    spc = std::min<int64_t>(n_sub, std::max<int64_t>(warm_sub + 1, cdiv(n_sub, cdiv(SOS_BANK_WAVES, b->C))));
  }
  const int64_t chunks = n_sub > 0 ? cdiv(n_sub, spc) : 1;
  const float *st_in = b->st[b->cur];
  float *st_out = b->st[b->cur ^ 1];
  for (int64_t c0 = 0; c0 < b->C; c0 += b->ymax) {
    const unsigned cy = (unsigned) std::min<int64_t>(b->ymax, b->C - c0);
    if (nch == 1)
      hipLaunchKernelGGL(sos_bank_kernel<1>, dim3((unsigned) chunks, cy), dim3(64), 0, st, x, ldx_f, y, ldy_f, s->d_sec, s->nsec,
                         s->gain, st_in, st_out, nfl, (int) spc, (int) warm_sub, (int) warm_nar, c0);
    else
      hipLaunchKernelGGL(sos_bank_kernel<2>, dim3((unsigned) chunks, cy), dim3(64), 0, st, x, ldx_f, y, ldy_f, s->d_sec, s->nsec,
                         s->gain, st_in, st_out, nfl, (int) spc, (int) warm_sub, (int) warm_nar, c0);
    TSD_HIP(hipGetLastError());
  }
  return TSDGPU_OK;
}

// Long blocks: channel after channel through tsdgpu_sos_step (its planner, the exact carry included), the handle's two state
// slots pointed at the channel's two records for the call.  The new state ends in b->st[cur ^ 1] for every channel.
int sos_bank_by_channel(tsdgpu_sos_bank *b, const char *x, int64_t ldx, char *y, int64_t ldy, int64_t n, hipStream_t st)
{
  tsdgpu_sos *s = b->proto;
  const size_t sz = dtype_size(s->data_type);
  float *own[2] = {s->d_state[0], s->d_state[1]};
  const int own_cur = s->cur;
  int rc = TSDGPU_OK;
  for (int64_t c = 0; c < b->C && !rc; c++) {
    float *in = b->st[b->cur] + c * STATE_FLOATS, *out = b->st[b->cur ^ 1] + c * STATE_FLOATS;
    s->d_state[0] = in;
    s->d_state[1] = out;
    s->cur = 0;
    rc = tsdgpu_sos_step(s, x + (size_t) c * (size_t) ldx * sz, y + (size_t) c * (size_t) ldy * sz, n, st);
    if (!rc && s->cur == 0) rc = device_copy_small(out, in, STATE_FLOATS * sizeof(float), st);
  }
  s->d_state[0] = own[0];
  s->d_state[1] = own[1];
  s->cur = own_cur;
  return rc;
}

}  // namespace
}  // namespace tsdgpu

using namespace tsdgpu;

extern "C" {

// ------------------------------------------------------------------ FIR bank
int tsdgpu_fir_bank_create(tsdgpu_fir_bank **out, int data_type, int tap_type, const void *taps_host, int ntaps, int channels)
{
  return tsdgpu_fir_bank_create_method(out, data_type, tap_type, taps_host, ntaps, channels, TSDGPU_FIR_DIRECT);
}

int tsdgpu_fir_bank_create_method(tsdgpu_fir_bank **out, int data_type, int tap_type, const void *taps_host, int ntaps, int channels,
                                  int method)
{
  TSD_CHECK(out != nullptr, "fir_bank_create: out is NULL");
  *out = nullptr;
  TSD_CHECK(channels >= 1, "fir_bank_create: channels = %d, need at least one", channels);
  TSD_CHECK(method >= TSDGPU_FIR_AUTO && method <= TSDGPU_FIR_OVERLAP_SAVE, "fir_bank_create: bad method %d", method);
  if (ntaps > 12289)
    return set_err(TSDGPU_ERR_UNSUPPORTED, "fir_bank_create: %d taps, the bank's direct scheme serves up to 12289", ntaps);
  tsdgpu_fir_bank *b = new tsdgpu_fir_bank();
  b->C = channels;
  b->method = method;
  int rc = tsdgpu_fir_create(&b->proto, data_type, tap_type, taps_host, ntaps, TSDGPU_FIR_DIRECT);
  if (!rc) rc = grid_y_limit(&b->ymax);
  // the overlap-save plan inside its envelope (2 .. 961 taps); outside it the bank runs the direct scheme, as a single handle does
  if (!rc && method != TSDGPU_FIR_DIRECT) rc = ols_bank_plan(b->proto, &b->ols, &b->ols_grid);
  if (!rc) {
    b->HL = b->ols ? std::max(b->proto->HL, ols_bank_overlap(b->proto)) : b->proto->HL;
    const size_t hb = (size_t) channels * (size_t) b->HL * dtype_size(data_type);
    if (hipMalloc(&b->hist[0], 2 * hb) != hipSuccess) {
      rc = set_err(TSDGPU_ERR_ALLOC, "fir_bank_create: hipMalloc of %zu bytes failed: %s", 2 * hb, hipGetErrorString(hipGetLastError()));
    } else {
      b->hist[1] = (char *) b->hist[0] + hb;
      if (hipMemset(b->hist[0], 0, 2 * hb) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess)
        rc = set_err(TSDGPU_ERR_HIP, "fir_bank_create: clearing the histories failed: %s", hipGetErrorString(hipGetLastError()));
    }
  }
  if (rc) {
    tsdgpu_fir_bank_destroy(b);
    return rc;
  }
  *out = b;
  return TSDGPU_OK;
}

int tsdgpu_fir_bank_step(tsdgpu_fir_bank *b, const void *x, int64_t ldx, void *y, int64_t ldy, int64_t n, void *stream)
{
  TSD_CHECK(b != nullptr, "fir_bank_step: NULL handle");
  TSD_CHECK(n >= 0, "fir_bank_step: negative length");
  if (n == 0) return TSDGPU_OK;
  const size_t sz = dtype_size(b->proto->data_type);
  int rc = bank_step_checks("fir_bank_step", x, ldx, y, ldy, n, b->C, sz);
  if (rc) return rc;
  hipStream_t st = (hipStream_t) stream;
  // in place: tiles read their neighbours' inputs, so filter from a private copy (as tsdgpu_fir_step does)
  const bool in_place = x == y;
  const void *dx;
  void *dy;
  int64_t dldx, dldy;
  bool staged;
  if ((rc = bank_stage_in(x, ldx, n, b->C, sz, in_place, n, b->in_stage, st, &dx, &dldx))) return rc;
  if ((rc = bank_stage_out(y, ldy, b->C, sz, false, n, b->out_stage, &dy, &dldy, &staged))) return rc;
  // the scheme of this step: AUTO decides per step (the channel length matters as much as the tap count)
  const bool ols = b->ols && (b->method == TSDGPU_FIR_OVERLAP_SAVE || ols_bank_preferred(b->proto, n));
  if (ols) rc = ols_bank_launch(b->proto, b->ols_grid, b->C, dx, dldx, dy, dldy, n, b->hist[b->cur], b->hist[b->cur ^ 1], b->HL, st);
  else if (b->proto->data_type == TSDGPU_F32) rc = fir_bank_launch<float, float, 16>(b, dx, dldx, dy, dldy, n, st);
  else if (b->proto->tap_type == TSDGPU_F32) rc = fir_bank_launch<float2, float, 8>(b, dx, dldx, dy, dldy, n, st);
  else rc = fir_bank_launch<float2, float2, 8>(b, dx, dldx, dy, dldy, n, st);
  if (rc) return rc;
  b->cur ^= 1;
  b->last = ols ? TSDGPU_FIR_OVERLAP_SAVE : TSDGPU_FIR_DIRECT;
  b->stepped = true;
  return bank_finish_out(y, ldy, n, b->C, sz, dy, dldy, staged, st);
}

int tsdgpu_fir_bank_method_used(const tsdgpu_fir_bank *b)
{
  if (!b) return -1;
  if (b->stepped) return b->last;
  return b->ols && (b->method == TSDGPU_FIR_OVERLAP_SAVE || ols_bank_preferred(b->proto, 1024)) ? TSDGPU_FIR_OVERLAP_SAVE : TSDGPU_FIR_DIRECT;
}

int tsdgpu_fir_bank_reset(tsdgpu_fir_bank *b)
{
  TSD_CHECK(b != nullptr, "fir_bank_reset: NULL handle");
  TSD_HIP(hipMemset(b->hist[b->cur], 0, (size_t) b->C * (size_t) b->HL * dtype_size(b->proto->data_type)));
  TSD_HIP(hipStreamSynchronize(nullptr));      // see tsdgpu_sos_reset
  return TSDGPU_OK;
}

// channels x (ntaps - 1) samples, channel-major, oldest first: the (ntaps - 1)-sample tail of every history row
int tsdgpu_fir_bank_get_history(tsdgpu_fir_bank *b, void *dst, void *stream)
{
  TSD_CHECK(b != nullptr && dst != nullptr, "fir_bank_get_history: NULL argument");
  const int K1 = b->proto->K - 1, HL = b->HL;
  if (K1 < 1) return TSDGPU_OK;
  hipStream_t st = (hipStream_t) stream;
  const size_t sz = dtype_size(b->proto->data_type);
  const char *src = (const char *) b->hist[b->cur] + (size_t) (HL - K1) * sz;
  const bool dev = is_device_ptr(dst);
  TSD_HIP(hipMemcpy2DAsync(dst, (size_t) K1 * sz, src, (size_t) HL * sz, (size_t) K1 * sz, (size_t) b->C,
                           dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  if (!dev) TSD_HIP(hipStreamSynchronize(st));
  return TSDGPU_OK;
}

int tsdgpu_fir_bank_set_history(tsdgpu_fir_bank *b, const void *src, void *stream)
{
  TSD_CHECK(b != nullptr && src != nullptr, "fir_bank_set_history: NULL argument");
  const int K1 = b->proto->K - 1, HL = b->HL;
  if (K1 < 1) return TSDGPU_OK;
  hipStream_t st = (hipStream_t) stream;
  const size_t sz = dtype_size(b->proto->data_type);
  char *dst = (char *) b->hist[b->cur] + (size_t) (HL - K1) * sz;
  const bool dev = is_device_ptr(src);
  TSD_HIP(hipMemcpy2DAsync(dst, (size_t) HL * sz, src, (size_t) K1 * sz, (size_t) K1 * sz, (size_t) b->C,
                           dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  if (!dev) TSD_HIP(hipStreamSynchronize(st));  // (`src` may die with the caller's scope)
  return TSDGPU_OK;
}

int tsdgpu_fir_bank_destroy(tsdgpu_fir_bank *b)
{
  if (!b) return TSDGPU_OK;
  if (b->hist[0]) (void) hipFree(b->hist[0]);   // (both histories live in the same allocation)
  tsdgpu_fir_destroy(b->proto);
  b->in_stage.release();
  b->out_stage.release();
  delete b;
  return TSDGPU_OK;
}

// ------------------------------------------------------------------ SOS bank
int tsdgpu_sos_bank_create(tsdgpu_sos_bank **out, int data_type, const float *coefs_host, int nsec, float gain,
                           const float *rii1_host, int forme, int channels)
{
  TSD_CHECK(out != nullptr, "sos_bank_create: out is NULL");
  *out = nullptr;
  TSD_CHECK(channels >= 1, "sos_bank_create: channels = %d, need at least one", channels);
  tsdgpu_sos_bank *b = new tsdgpu_sos_bank();
  b->C = channels;
  int rc = tsdgpu_sos_create(&b->proto, data_type, coefs_host, nsec, gain, rii1_host, forme);
  if (!rc) rc = grid_y_limit(&b->ymax);
  if (!rc) {
    const size_t sb = (size_t) channels * STATE_FLOATS * sizeof(float);
    if (hipMalloc((void **) &b->st[0], 2 * sb) != hipSuccess) {
      rc = set_err(TSDGPU_ERR_ALLOC, "sos_bank_create: hipMalloc of %zu bytes failed: %s", 2 * sb, hipGetErrorString(hipGetLastError()));
    } else {
      b->st[1] = b->st[0] + (size_t) channels * STATE_FLOATS;
      if (hipMemset(b->st[0], 0, 2 * sb) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess)
        rc = set_err(TSDGPU_ERR_HIP, "sos_bank_create: clearing the states failed: %s", hipGetErrorString(hipGetLastError()));
    }
  }
  if (rc) {
    tsdgpu_sos_bank_destroy(b);
    return rc;
  }
  *out = b;
  return TSDGPU_OK;
}

int tsdgpu_sos_bank_step(tsdgpu_sos_bank *b, const void *x, int64_t ldx, void *y, int64_t ldy, int64_t n, void *stream)
{
  TSD_CHECK(b != nullptr, "sos_bank_step: NULL handle");
  TSD_CHECK(n >= 0, "sos_bank_step: negative length");
  if (n == 0) return TSDGPU_OK;
  const size_t sz = dtype_size(b->proto->data_type);
  int rc = bank_step_checks("sos_bank_step", x, ldx, y, ldy, n, b->C, sz);
  if (rc) return rc;
  hipStream_t st = (hipStream_t) stream;
  const int64_t q = 16 / (int64_t) sz;                      // samples per 16 B
  const int64_t ld_s = cdiv(n, q) * q;                      // packed rows of the staging buffers, 16-B aligned
  const bool by_channel = n >= SOS_BANK_SINGLE_MIN;
  // the wave kernel moves 16 B per lane from 16-B aligned rows: other rows are bounced through packed aligned ones (the
  // single-stream step bounces misaligned vectors itself); in place, chunks re-read their predecessors' inputs (warm-ups)
  auto aligned = [&](const void *p, int64_t ld) { return by_channel || ((((uintptr_t) p & 15) == 0) && ((ld * (int64_t) sz) % 16 == 0)); };
  const bool in_place = x == y;
  const void *dx;
  void *dy;
  int64_t dldx, dldy;
  bool staged;
  if ((rc = bank_stage_in(x, ldx, n, b->C, sz, in_place || !aligned(x, ldx), ld_s, b->in_stage, st, &dx, &dldx))) return rc;
  if ((rc = bank_stage_out(y, ldy, b->C, sz, !aligned(y, ldy), ld_s, b->out_stage, &dy, &dldy, &staged))) return rc;
  if (by_channel) {
    rc = sos_bank_by_channel(b, (const char *) dx, dldx, (char *) dy, dldy, n, st);
  } else {
    const int64_t f = (int64_t) sz / 4;                     // floats per sample
    rc = sos_bank_launch(b, (const float *) dx, dldx * f, (float *) dy, dldy * f, n, st);
  }
  if (rc) return rc;
  b->cur ^= 1;
  return bank_finish_out(y, ldy, n, b->C, sz, dy, dldy, staged, st);
}

int tsdgpu_sos_bank_reset(tsdgpu_sos_bank *b)
{
  TSD_CHECK(b != nullptr, "sos_bank_reset: NULL handle");
  TSD_HIP(hipMemset(b->st[b->cur], 0, (size_t) b->C * STATE_FLOATS * sizeof(float)));
  TSD_HIP(hipStreamSynchronize(nullptr));      // see tsdgpu_sos_reset
  return TSDGPU_OK;
}

int tsdgpu_sos_bank_get_state(tsdgpu_sos_bank *b, int channel, float *state_host, void *stream)
{
  TSD_CHECK(b != nullptr && state_host != nullptr, "sos_bank_get_state: NULL argument");
  TSD_CHECK(channel >= 0 && channel < b->C, "sos_bank_get_state: channel %d outside [0, %lld)", channel, (long long) b->C);
  hipStream_t st = (hipStream_t) stream;
  TSD_HIP(hipMemcpyAsync(state_host, b->st[b->cur] + (size_t) channel * STATE_FLOATS, STATE_FLOATS * sizeof(float),
                         hipMemcpyDeviceToHost, st));
  TSD_HIP(hipStreamSynchronize(st));
  return TSDGPU_OK;
}

int tsdgpu_sos_bank_set_state(tsdgpu_sos_bank *b, int channel, const float *state_host, void *stream)
{
  TSD_CHECK(b != nullptr && state_host != nullptr, "sos_bank_set_state: NULL argument");
  TSD_CHECK(channel >= 0 && channel < b->C, "sos_bank_set_state: channel %d outside [0, %lld)", channel, (long long) b->C);
  hipStream_t st = (hipStream_t) stream;
  TSD_HIP(hipMemcpyAsync(b->st[b->cur] + (size_t) channel * STATE_FLOATS, state_host, STATE_FLOATS * sizeof(float),
                         hipMemcpyHostToDevice, st));
  TSD_HIP(hipStreamSynchronize(st));            // (`state_host` may die with the caller's scope)
  return TSDGPU_OK;
}

int tsdgpu_sos_bank_destroy(tsdgpu_sos_bank *b)
{
  if (!b) return TSDGPU_OK;
  if (b->st[0]) (void) hipFree(b->st[0]);       // (both state arrays live in the same allocation)
  tsdgpu_sos_destroy(b->proto);
  b->in_stage.release();
  b->out_stage.release();
  delete b;
  return TSDGPU_OK;
}

}  // extern "C"
