// rate_bank.hip -- C-channel bank of the integer-rate stages: many streams through ONE decimator / half-band / upsampler /
// pick in one launch per step.
//
// Stands behind FiltreRIFDecim / FiltreRIFDemiBande / FiltreRIFUps (libtsd core/src/reechan/polyphase.cc:54-341) and
// Decimateur (core/src/filtrage/filtre-rt.cc:127-169) applied to every column of an n x C column-major Tab.  Channel c of a
// step reads x + c ldx (n samples) and writes y + c ldy (the same number of outputs in every channel: the bank has ONE phase
// counter, the single handle's `cnt`); only the history rows are per channel.  Every channel is bit-identical to its own
// tsdgpu_polyfir handle fed the same blocks wherever that handle runs its direct or fused kernel (polyphase.hip).
//
// Two arithmetic schemes on a (tile, channel) grid, chosen where the single-stream handle chooses them (poly_internal.hpp):
//  - direct scheme (decimators of rate 2 / 4 / 8 up to 64 taps, upsamplers of rate 2 / 4 with branches up to 32 taps):
//    decim_direct_kernel / ups_direct_kernel's lane layout -- a lane owns a 64-B segment of input positions, segments 80 B
//    apart in LDS, a two-segment register window slides over the reversed, zero-padded taps (wave-uniform loads) -- staged
//    as fir_bank_kernel stages: 16-B loads for every unit inside the channel's block, the halo of the first tile from the
//    channel's history row, zeros past the end; lanes wholly past the end skip their multiply-adds.  One wave per workgroup;
//    channels shorter than a wave's 64 segments share the wave.
//  - oldest-first scheme (everything else): polyfir_fused_kernel's chain acc = fma(g[k], x[newest - k], acc), k = W-1 .. 0.
// The last tile of a channel writes the channel's new history row into the other buffer in the same launch.
#include "common.hpp"
#include "poly_internal.hpp"
#include "bank_internal.hpp"
#include <algorithm>
#include <vector>

struct tsdgpu_polyfir_bank {
  int kind = 0, data_type = 0, R = 1, K = 0;
  int64_t C = 0;
  int cnt = 0;                     // the common phase counter: inputs seen since the last kept output (decimators / pick)
  int NPH = 1, W = 0, stride = 1;  // the stage in the terms of poly_internal.hpp
  int HW = 0;                      // history samples per channel (0: pick)
  int TO = 0;                      // oldest-first scheme: outputs per workgroup
  int KPd = 0;                     // direct scheme: length of a padded tap row (0: oldest-first scheme)
  float *d_g = nullptr;            // taps [NPH][W], then the direct scheme's rows [NPH][KPd] (one allocation)
  float *d_hrev = nullptr;
  void *hist[2] = {nullptr, nullptr};   // C rows of HW samples, oldest first (double-buffered, one allocation)
  int cur = 0;
  int ymax = 0;                    // the grid's y limit (channels per launch)
  tsdgpu::DevBuf in_stage, out_stage;
};

namespace tsdgpu {
namespace {

__device__ __forceinline__ float rb_mac(float acc, float g, float x) { return fmaf(g, x, acc); }
__device__ __forceinline__ float2 rb_mac(float2 acc, float g, float2 x) { return make_float2(fmaf(g, x.x, acc.x), fmaf(g, x.y, acc.y)); }
__device__ __forceinline__ float rb_zero(float) { return 0.f; }
__device__ __forceinline__ float2 rb_zero(float2) { return make_float2(0.f, 0.f); }

// the channel's new history: the last HW samples of (old history ++ x[0, n))
template <typename T>
__device__ __forceinline__ void rb_write_history(const T *__restrict__ x, const T *__restrict__ oh, T *__restrict__ nh, int HW, int64_t n)
{
  for (int i = threadIdx.x; i < HW; i += blockDim.x) {
    const int64_t g = n - HW + i;
    nh[i] = g < 0 ? oh[HW + g] : x[g];
  }
}

// ------------------------------------------------------------------ direct scheme
// DEC > 1, RU = 1: decimator, a tile starts on the kept position `start` + blockIdx.x TILE and a lane keeps the positions
// r = 0, DEC, 2 DEC ... of its segment.  DEC = 1, RU > 1: upsampler, RU branch rows of hrev, RU outputs per position.
// Lane window: w[i] = sample t RS + 1 + i of the staged tile; out(position r, branch i) = sum_j hrev[i][j] w[r + j], j
// ascending: oldest sample first, the zero-padded head of the row first.
// One wave per workgroup.  LPC = 1 << lsh lanes serve one channel (a tile of LPC lane segments), so a wave serves G = 64 / LPC
// channels: c0 + blockIdx.y G + (lane / LPC).  Long channels: LPC = 64, tile after tile along blockIdx.x; channels shorter than
// a wave's 64 segments share the wave (LPC = 8 .. 32).  Each channel of the wave has its own LDS region of `region` samples,
// a whole number of 16 segments, so that the lanes of one ds_read_b128 group keep distinct banks across regions.
template <typename T, int RS, int DEC, int RU, bool AL>
__global__ __launch_bounds__(64) void rate_bank_direct_kernel(const T *__restrict__ x, int64_t ldx, T *__restrict__ y, int64_t ldy,
                                                              const float *__restrict__ hrev, int KP, int start, int64_t n, int64_t nout,
                                                              const T *__restrict__ old_hist, T *__restrict__ new_hist, int HW, int64_t c0,
                                                              int64_t C, int lsh, int region)
{
  constexpr int VEC = 16 / (int) sizeof(T), P = VEC, SP = RS + P;
  constexpr int RO = RS / DEC;                       // kept positions per lane
  constexpr int NO = RO * RU;                        // outputs per lane (contiguous in y)
  constexpr int OS = NO % VEC == 0 ? NO + VEC : NO;  // their pitch in LDS: an odd number of 16-B units, or packed when below one unit
  static_assert(RS * sizeof(T) == 64 && RS % DEC == 0, "one lane segment is 64 bytes, a whole number of kept positions");
  static_assert(DEC == 1 || RU == 1, "a decimator or an upsampler");
  static_assert((8 * NO) % VEC == 0, "tiles (8 lanes or more) start on a 16-B unit of the output row");
  extern __shared__ __attribute__((aligned(16))) char rbd_raw[];
  T *L = reinterpret_cast<T *>(rbd_raw);

  const int LPC = 1 << lsh, TILE = RS << lsh, TILE_OUT = NO << lsh;
  const int64_t chg = c0 + ((int64_t) blockIdx.y << (6 - lsh));             // first channel of the wave
  const int gmax = (int) min((int64_t) (64 >> lsh), C - chg);               // channels of the wave
  const int grp = threadIdx.x >> lsh, tl = threadIdx.x & (LPC - 1);         // the lane's channel and its segment in the tile
  const int64_t tile0 = (int64_t) start + (int64_t) blockIdx.x * TILE;      // first position of the tile
  const int H = KP, total = TILE + H;                                       // staged samples 1 .. total - 1: position tile0 - H + s

  // the last tile of a channel writes the channel's new history row into the other buffer
  if (blockIdx.x == gridDim.x - 1 && grp < gmax) {
    const int64_t ch = chg + grp;
    const T *xc = x + ch * ldx, *oh = old_hist + ch * HW;
    T *nh = new_hist + ch * HW;
    for (int i = tl; i < HW; i += LPC) {
      const int64_t g = n - HW + i;
      nh[i] = g < 0 ? oh[HW + g] : xc[g];
    }
  }

  // chunk c = staged samples [c VEC + 1, c VEC + 1 + VEC) of a channel: one 16-B load when the unit lies inside [0, n), else
  // element by element from the history (before 0; zeros before the history: the padded taps meet those) or zeros (from n on)
  const int nchunks = (total - 1 + VEC - 1) / VEC, all = gmax * nchunks;
  for (int f0 = threadIdx.x; f0 < all; f0 += 4 * 64) {
    f4u q4[4];
    int dst[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int f = f0 + u * 64;
      if (f < all) {
        const int gq = f / nchunks, c = f - gq * nchunks, q = c * VEC;
        dst[u] = gq * region + q + (q / RS) * P;
        const int64_t ch = chg + gq;
        const T *xc = x + ch * ldx;
        const int64_t g0 = tile0 - H + 1 + (int64_t) q;
        if (g0 >= 0 && g0 + VEC <= n) {
          q4[u] = *reinterpret_cast<const f4u *>(xc + g0);
        } else {
          const T *oh = old_hist + ch * HW;
          T *e = reinterpret_cast<T *>(&q4[u]);
#pragma unroll
          for (int k = 0; k < VEC; k++) {
            const int64_t g = g0 + k;
            e[k] = g < 0 ? (g >= -(int64_t) HW ? oh[HW + g] : rb_zero(T{})) : g < n ? xc[g] : rb_zero(T{});
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (f0 + u * 64 < all) *reinterpret_cast<float4 *>(L + dst[u]) = make_float4(q4[u].x, q4[u].y, q4[u].z, q4[u].w);
  }
  __syncthreads();

  T *Lg = L + grp * region;
  const T *Lw = Lg + tl * SP;
  T acc[RU][RO], A[RS], B[RS];
  auto load_seg = [&](T (&dst)[RS], const T *seg) {
#pragma unroll
    for (int v4 = 0; v4 < RS / VEC; v4++) {
      const float4 q4 = *reinterpret_cast<const float4 *>(seg + v4 * VEC);
      const T *e = reinterpret_cast<const T *>(&q4);
#pragma unroll
      for (int k = 0; k < VEC; k++) dst[v4 * VEC + k] = e[k];
    }
  };
#pragma unroll
  for (int i = 0; i < RU; i++)
#pragma unroll
    for (int r = 0; r < RO; r++) acc[i][r] = rb_zero(T{});
  if (grp < gmax && tile0 + (int64_t) tl * RS < n) {         // (lanes wholly past the channel's end have nothing to compute)
    load_seg(A, Lw);
    const int nchunk = KP / RS;                              // even by construction
    for (int c = 0; c < nchunk; c += 2) {
      load_seg(B, Lw + (c + 1) * SP);
#pragma unroll
      for (int jj = 0; jj < RS; jj++)
#pragma unroll
        for (int i = 0; i < RU; i++) {
          const float hv = hrev[i * KP + c * RS + jj];
#pragma unroll
          for (int r = 0; r < RO; r++) {
            const int idx = r * DEC + jj;
            acc[i][r] = rb_mac(acc[i][r], hv, idx < RS ? A[idx] : B[idx - RS]);
          }
        }
      load_seg(A, Lw + (c + 2) * SP);                        // (the last refill reads two over-allocated segments, never used)
#pragma unroll
      for (int jj = 0; jj < RS; jj++)
#pragma unroll
        for (int i = 0; i < RU; i++) {
          const float hv = hrev[i * KP + (c + 1) * RS + jj];
#pragma unroll
          for (int r = 0; r < RO; r++) {
            const int idx = r * DEC + jj;
            acc[i][r] = rb_mac(acc[i][r], hv, idx < RS ? B[idx] : A[idx - RS]);
          }
        }
    }
  }

  // the lane's NO outputs (position-major, branch-minor) back through LDS; whole 16-B units of a channel's output row go
  // out as 16-B stores, its last partial unit element by element
  __syncthreads();
  T *Lo = Lg + tl * OS;
#pragma unroll
  for (int r = 0; r < RO; r++)
#pragma unroll
    for (int i = 0; i < RU; i++) Lo[r * RU + i] = acc[i][r];
  __syncthreads();
  const int64_t ob = (int64_t) blockIdx.x * TILE_OUT;
  const int ush = lsh + __builtin_ctz(NO) - __builtin_ctz(VEC);             // log2 of the 16-B units of a channel's tile
  for (int f = threadIdx.x; f < (gmax << ush); f += 64) {
    const int gq = f >> ush, e0 = (f & ((1 << ush) - 1)) * VEC;
    const int64_t o = ob + e0;
    if (o >= nout) continue;
    T *yc = y + (chg + gq) * ldy;
    const float4 q4 = *reinterpret_cast<const float4 *>(L + gq * region + (e0 / NO) * OS + (e0 % NO));
    if (o + VEC <= nout) {
      if (AL) *reinterpret_cast<float4 *>(yc + o) = q4;
      else *reinterpret_cast<f4u *>(yc + o) = f4u{q4.x, q4.y, q4.z, q4.w};
    } else {
      const T *e = reinterpret_cast<const T *>(&q4);
      for (int k = 0; k < VEC && o + k < nout; k++) yc[o + k] = e[k];
    }
  }
}

// ------------------------------------------------------------------ oldest-first scheme
// polyfir_fused_kernel on the (tile, channel) grid: a workgroup stages the input span of its TO outputs (8 loads in flight
// per thread) and the taps in LDS; output o = grp NPH + ph is the ONE chain
//     acc = 0; for k = W-1 .. 0: acc = fma(g[ph][k], x[grp stride + start - k], acc).
template <typename T>
__global__ __launch_bounds__(256) void rate_bank_fused_kernel(const T *__restrict__ x, int64_t ldx, T *__restrict__ y, int64_t ldy,
                                                              const float *__restrict__ g, int NPH, int W, int stride, int64_t start,
                                                              int64_t n, int64_t nout, int TO, const T *__restrict__ old_hist,
                                                              T *__restrict__ new_hist, int HW, int64_t c0)
{
  extern __shared__ __attribute__((aligned(16))) char rbf_raw[];
  float *gs = reinterpret_cast<float *>(rbf_raw);                        // NPH * W taps
  T *xs = reinterpret_cast<T *>(gs + ((NPH * W + 3) & ~3));              // staged inputs
  const int t = threadIdx.x;
  const int64_t ch = c0 + blockIdx.y;
  x += ch * ldx;
  y += ch * ldy;
  const T *oh = old_hist + ch * HW;
  if (blockIdx.x == gridDim.x - 1) rb_write_history(x, oh, new_hist + ch * HW, HW, n);
  const int64_t o0 = (int64_t) blockIdx.x * TO;
  const int64_t o1 = min(o0 + TO, nout);                              // exclusive
  if (o0 >= o1) return;                                               // (a step without outputs: only the history moves)
  for (int i = t; i < NPH * W; i += 256) gs[i] = g[i];
  const int64_t grp0 = o0 / NPH, grp1 = (o1 - 1) / NPH;
  const int64_t i_lo = grp0 * stride + start - (W - 1), i_hi = grp1 * stride + start;   // inclusive input span
  const int span = (int) (i_hi - i_lo + 1);
  for (int i0 = t; i0 < span; i0 += 256 * 8) {
    T v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int i = i0 + 256 * u;
      const int64_t idx = i_lo + i;
      v[u] = rb_zero(T{});
      if (i < span) {
        if (idx < 0) {
          if (idx >= -(int64_t) HW) v[u] = oh[HW + idx];
        } else if (idx < n) {
          v[u] = x[idx];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int i = i0 + 256 * u;
      if (i < span) xs[i] = v[u];
    }
  }
  __syncthreads();
  for (int64_t o = o0 + t; o < o1; o += 256) {
    const int64_t grp = o / NPH;
    const int ph = (int) (o - grp * NPH);
    const int b = (int) (grp * stride + start - i_lo);                   // staged index of the newest sample
    const float *gp = gs + ph * W;
    T acc = rb_zero(T{});
    for (int k = W - 1; k >= 0; k--) acc = rb_mac(acc, gp[k], xs[b - k]);   // oldest sample first, like the reference
    y[o] = acc;
  }
}

// ------------------------------------------------------------------ Decimateur: y[c][m] = x[c][start + m R]
template <typename T>
__global__ __launch_bounds__(256) void rate_bank_pick_kernel(const T *__restrict__ x, int64_t ldx, T *__restrict__ y, int64_t ldy,
                                                             int64_t start, int R, int64_t nout, int64_t c0)
{
  const int64_t ch = c0 + blockIdx.y;
  const int64_t m = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (m < nout) y[ch * ldy + m] = x[ch * ldx + start + m * R];
}

// One wave per workgroup (64 lane segments = 4 KiB of input): against the single-stream kernels' 256 lanes, 2.0-2.7 x faster at
// n = 512 (a 256-lane tile is mostly idle lanes there) and 0-12 % faster at n = 4096 and 65536 -- more workgroups per CU in
// different phases of load / multiply / store, and barriers that a single wave does not wait at (EXPERIMENTS.md).  Channels
// shorter than the wave's tile share it -- the fewest lanes per channel, 8 at least, whose segments cover the block: against one
// channel per wave 4.5 x faster at n = 64, 2.3-3.9 x at 128, 1.35-2.2 x at 256, 1.4 x for floats at 512, equal from 1024 on.
template <typename T, int RS, int DEC, int RU>
int direct_launch(tsdgpu_polyfir_bank *b, const void *x, int64_t ldx, void *y, int64_t ldy, int start, int64_t n, int64_t nout, hipStream_t st)
{
  constexpr int VEC = 16 / (int) sizeof(T), SP = RS + VEC, NO = RS / DEC * RU, OS = NO % VEC == 0 ? NO + VEC : NO;
  int lsh = 6;
  while (lsh > 3 && ((int64_t) RS << (lsh - 1)) >= n) lsh--;
  const int LPC = 1 << lsh, G = 64 >> lsh, TILE = RS << lsh;
  const int64_t tiles = std::max<int64_t>(1, DEC > 1 ? cdiv(nout, TILE / DEC) : cdiv(n, TILE));
  if (tiles > 0x7fffffff) return set_err(TSDGPU_ERR_UNSUPPORTED, "polyfir_bank_step: n = %lld too large for one launch", (long long) n);
  // a channel's LDS region: the staged tile ((TILE + KP) / RS + 3 segments) or the lanes' outputs, in whole groups of 16 segments
  const int segs = (int) cdiv(std::max<int64_t>((TILE + b->KPd) / RS + 3, cdiv((int64_t) LPC * OS, SP)), 16) * 16, region = segs * SP;
  const size_t lds = (size_t) G * region * sizeof(T);       // (at most 20 KiB)
  const T *oldh = (const T *) b->hist[b->cur];
  T *newh = (T *) b->hist[b->cur ^ 1];
  const bool al = ((uintptr_t) y & 15) == 0 && (ldy * (int64_t) sizeof(T)) % 16 == 0;
  const int64_t per_launch = (int64_t) b->ymax * G;
  for (int64_t c0 = 0; c0 < b->C; c0 += per_launch) {
    const unsigned cy = (unsigned) cdiv(std::min<int64_t>(per_launch, b->C - c0), G);
    if (al)
      hipLaunchKernelGGL((rate_bank_direct_kernel<T, RS, DEC, RU, true>), dim3((unsigned) tiles, cy), dim3(64), lds, st, (const T *) x, ldx,
                         (T *) y, ldy, b->d_hrev, b->KPd, start, n, nout, oldh, newh, b->HW, c0, b->C, lsh, region);
    else
      hipLaunchKernelGGL((rate_bank_direct_kernel<T, RS, DEC, RU, false>), dim3((unsigned) tiles, cy), dim3(64), lds, st, (const T *) x, ldx,
                         (T *) y, ldy, b->d_hrev, b->KPd, start, n, nout, oldh, newh, b->HW, c0, b->C, lsh, region);
    TSD_HIP(hipGetLastError());
  }
  return TSDGPU_OK;
}

template <typename T>
int fused_launch(tsdgpu_polyfir_bank *b, const void *x, int64_t ldx, void *y, int64_t ldy, int64_t start, int64_t n, int64_t nout, hipStream_t st)
{
  // short channels: a workgroup's LDS follows the outputs there are (the bits do not depend on the cut in workgroups)
  const int TO = (int) std::min<int64_t>(b->TO, std::max<int64_t>(256, cdiv(nout, 256) * 256));
  const int64_t tiles = std::max<int64_t>(1, cdiv(nout, TO));
  if (tiles > 0x7fffffff) return set_err(TSDGPU_ERR_UNSUPPORTED, "polyfir_bank_step: n = %lld too large for one launch", (long long) n);
  const int64_t span = (int64_t) (TO / b->NPH + 1) * b->stride + b->W;
  const size_t lds = (size_t) ((b->NPH * b->W + 3) & ~3) * sizeof(float) + (size_t) span * sizeof(T);
  if (lds > 48 * 1024)
    (void) hipFuncSetAttribute((const void *) rate_bank_fused_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  for (int64_t c0 = 0; c0 < b->C; c0 += b->ymax) {
    const unsigned cy = (unsigned) std::min<int64_t>(b->ymax, b->C - c0);
    hipLaunchKernelGGL(rate_bank_fused_kernel<T>, dim3((unsigned) tiles, cy), dim3(256), lds, st, (const T *) x, ldx, (T *) y, ldy, b->d_g,
                       b->NPH, b->W, b->stride, start, n, nout, TO, (const T *) b->hist[b->cur], (T *) b->hist[b->cur ^ 1], b->HW, c0);
    TSD_HIP(hipGetLastError());
  }
  return TSDGPU_OK;
}

template <typename T>
int pick_launch(tsdgpu_polyfir_bank *b, const void *x, int64_t ldx, void *y, int64_t ldy, int64_t start, int64_t nout, hipStream_t st)
{
  if (nout <= 0) return TSDGPU_OK;
  for (int64_t c0 = 0; c0 < b->C; c0 += b->ymax) {
    const unsigned cy = (unsigned) std::min<int64_t>(b->ymax, b->C - c0);
    hipLaunchKernelGGL(rate_bank_pick_kernel<T>, dim3((unsigned) cdiv(nout, 256), cy), dim3(256), 0, st, (const T *) x, ldx, (T *) y, ldy,
                       start, b->R, nout, c0);
    TSD_HIP(hipGetLastError());
  }
  return TSDGPU_OK;
}

template <typename T>
int stage_launch(tsdgpu_polyfir_bank *b, const void *x, int64_t ldx, void *y, int64_t ldy, int64_t n, int64_t nout, hipStream_t st)
{
  constexpr int RS = 64 / (int) sizeof(T);
  if (b->kind == TSDGPU_POLY_PICK) return pick_launch<T>(b, x, ldx, y, ldy, b->cnt, nout, st);   // Decimateur picks x[cnt], x[cnt + R] ...
  // decimators: kept outputs sit at local inputs R - 1 - cnt, then every R; upsampler: group = input index
  const int start = b->kind == TSDGPU_POLY_UPS ? 0 : b->R - 1 - b->cnt;
  if (!b->KPd) return fused_launch<T>(b, x, ldx, y, ldy, start, n, nout, st);
  if (b->NPH == 2) return direct_launch<T, RS, 1, 2>(b, x, ldx, y, ldy, 0, n, nout, st);
  if (b->NPH == 4) return direct_launch<T, RS, 1, 4>(b, x, ldx, y, ldy, 0, n, nout, st);
  if (b->stride == 2) return direct_launch<T, RS, 2, 1>(b, x, ldx, y, ldy, start, n, nout, st);
  if (b->stride == 4) return direct_launch<T, RS, 4, 1>(b, x, ldx, y, ldy, start, n, nout, st);
  return direct_launch<T, RS, 8, 1>(b, x, ldx, y, ldy, start, n, nout, st);
}

int64_t bank_out_count(const tsdgpu_polyfir_bank *b, int64_t n)
{
  switch (b->kind) {
    case TSDGPU_POLY_DECIM:
    case TSDGPU_POLY_HALFBAND: return (n + b->cnt) / b->R;
    case TSDGPU_POLY_UPS: return n * b->R;
    default: return (n + b->R - 1 - b->cnt) / b->R;      // Decimateur (filtre-rt.cc:139)
  }
}

size_t hist_bytes(const tsdgpu_polyfir_bank *b) { return (size_t) b->C * (size_t) b->HW * dtype_size(b->data_type); }

}  // namespace
}  // namespace tsdgpu

using namespace tsdgpu;

extern "C" {

int tsdgpu_polyfir_bank_create(tsdgpu_polyfir_bank **out, int kind, int data_type, const float *taps_host, int ntaps, int R, int channels)
{
  TSD_CHECK(out != nullptr, "polyfir_bank_create: out is NULL");
  *out = nullptr;
  TSD_CHECK(kind >= TSDGPU_POLY_DECIM && kind <= TSDGPU_POLY_PICK, "polyfir_bank_create: bad kind %d", kind);
  TSD_CHECK(data_type == TSDGPU_F32 || data_type == TSDGPU_C64, "polyfir_bank_create: bad data_type %d", data_type);
  if (kind == TSDGPU_POLY_HALFBAND) R = 2;
  TSD_CHECK(R >= 1 && R <= 4096, "polyfir_bank_create: bad rate %d", R);
  TSD_CHECK(kind == TSDGPU_POLY_PICK || (taps_host != nullptr && ntaps > 0), "polyfir_bank_create: K > 0 required");
  TSD_CHECK(channels >= 1, "polyfir_bank_create: channels = %d, need at least one", channels);
  tsdgpu_polyfir_bank *b = new tsdgpu_polyfir_bank();
  b->kind = kind;
  b->data_type = data_type;
  b->R = R;
  b->K = kind == TSDGPU_POLY_PICK ? 0 : ntaps;
  b->C = channels;
  int rc = grid_y_limit(&b->ymax);
  if (!rc && kind != TSDGPU_POLY_PICK) {
    const PolyImage im = poly_tap_image(kind, taps_host, ntaps, R);
    if (!poly_fused_serves(im.NPH, im.W, im.stride)) {
      delete b;
      if ((size_t) im.NPH * im.W > 4096)
        return set_err(TSDGPU_ERR_UNSUPPORTED, "polyfir_bank_create: %d taps in %d branch(es): the bank keeps up to 4096 taps in LDS", im.NPH * im.W, im.NPH);
      return set_err(TSDGPU_ERR_UNSUPPORTED,
                     "polyfir_bank_create: rate %d with %d taps: the input span of a workgroup's 256 outputs (%lld samples) passes the %d samples staged in LDS",
                     R, ntaps, (long long) 257 * im.stride + im.W, PF_MAX_SPAN);
    }
    b->NPH = im.NPH;
    b->W = im.W;
    b->stride = im.stride;
    b->HW = std::max(im.W - 1, 1);
    b->TO = (int) (poly_fused_outputs(im.NPH, im.W, im.stride) / 256 * 256);
    b->KPd = poly_direct_regime(im.NPH, im.W, im.stride) ? poly_direct_kp(im.W, data_type) : 0;
    // one allocation and one upload for the taps and the direct scheme's rows; one allocation for the two history buffers
    const size_t gb = (im.g.size() * sizeof(float) + 15) / 16 * 16, rb = (size_t) b->KPd * im.NPH * sizeof(float);
    std::vector<char> image(gb + rb, 0);
    std::memcpy(image.data(), im.g.data(), im.g.size() * sizeof(float));
    if (b->KPd) poly_direct_rows(im.g, im.NPH, im.W, b->KPd, reinterpret_cast<float *>(image.data() + gb));
    const size_t hb = (hist_bytes(b) + 15) / 16 * 16;
    if (hipMalloc((void **) &b->d_g, image.size()) != hipSuccess || hipMalloc(&b->hist[0], 2 * hb) != hipSuccess) {
      rc = set_err(TSDGPU_ERR_ALLOC, "polyfir_bank_create: hipMalloc of %zu bytes failed: %s", image.size() + 2 * hb, hipGetErrorString(hipGetLastError()));
    } else {
      b->hist[1] = (char *) b->hist[0] + hb;
      b->d_hrev = b->KPd ? reinterpret_cast<float *>((char *) b->d_g + gb) : nullptr;
      if (hipMemcpy(b->d_g, image.data(), image.size(), hipMemcpyHostToDevice) != hipSuccess || hipMemset(b->hist[0], 0, 2 * hb) != hipSuccess ||
          hipStreamSynchronize(nullptr) != hipSuccess)
        rc = set_err(TSDGPU_ERR_HIP, "polyfir_bank_create: upload failed: %s", hipGetErrorString(hipGetLastError()));
    }
  }
  if (rc) {
    tsdgpu_polyfir_bank_destroy(b);
    return rc;
  }
  *out = b;
  return TSDGPU_OK;
}

int64_t tsdgpu_polyfir_bank_out_count(tsdgpu_polyfir_bank *b, int64_t n) { return (!b || n < 0) ? -1 : bank_out_count(b, n); }

int tsdgpu_polyfir_bank_step(tsdgpu_polyfir_bank *b, const void *x, int64_t ldx, int64_t n, void *y, int64_t ldy, int64_t y_capacity,
                             int64_t *n_out, void *stream)
{
  TSD_CHECK(b != nullptr, "polyfir_bank_step: NULL handle");
  TSD_CHECK(n >= 0, "polyfir_bank_step: negative length");
  if (n_out) *n_out = 0;
  if (n == 0) return TSDGPU_OK;
  const int64_t nout = bank_out_count(b, n);
  TSD_CHECK(x != nullptr && (nout == 0 || y != nullptr), "polyfir_bank_step: NULL buffer");
  TSD_CHECK(ldx >= n, "polyfir_bank_step: ldx = %lld below n = %lld", (long long) ldx, (long long) n);
  TSD_CHECK(nout <= y_capacity, "polyfir_bank_step: a channel's output needs %lld samples, y_capacity is %lld", (long long) nout,
            (long long) y_capacity);
  TSD_CHECK(ldy >= nout, "polyfir_bank_step: ldy = %lld below the %lld outputs of a channel", (long long) ldy, (long long) nout);
  hipStream_t st = (hipStream_t) stream;
  const size_t sz = dtype_size(b->data_type);
  // any overlap of the two footprints: work from a private copy of x (a decimator's tile t + 1 writes where tile t reads)
  const size_t ex = ((size_t) (b->C - 1) * (size_t) ldx + (size_t) n) * sz, ey = ((size_t) (b->C - 1) * (size_t) ldy + (size_t) nout) * sz;
  const bool overlap = nout > 0 && ranges_overlap(x, ex, y, ey);
  const void *dx;
  void *dy = nullptr;
  int64_t dldx, dldy = nout;
  bool staged = false;
  int rc;
  if ((rc = bank_stage_in(x, ldx, n, b->C, sz, overlap, n, b->in_stage, st, &dx, &dldx))) return rc;
  if (nout > 0 && (rc = bank_stage_out(y, ldy, b->C, sz, false, nout, b->out_stage, &dy, &dldy, &staged))) return rc;
  rc = b->data_type == TSDGPU_C64 ? stage_launch<float2>(b, dx, dldx, dy, dldy, n, nout, st) : stage_launch<float>(b, dx, dldx, dy, dldy, n, nout, st);
  if (rc) return rc;
  if (b->kind == TSDGPU_POLY_PICK) b->cnt = (int) (b->cnt + nout * b->R - n);      // new cnt = (first index >= n) - n
  else if (b->kind != TSDGPU_POLY_UPS) b->cnt = (int) ((b->cnt + n) % b->R);
  if (b->HW) b->cur ^= 1;
  if (n_out) *n_out = nout;
  return nout > 0 ? bank_finish_out(y, ldy, nout, b->C, sz, dy, dldy, staged, st) : TSDGPU_OK;
}

int tsdgpu_polyfir_bank_reset(tsdgpu_polyfir_bank *b)
{
  TSD_CHECK(b != nullptr, "polyfir_bank_reset: NULL handle");
  b->cnt = 0;
  if (b->HW) {
    TSD_HIP(hipMemset(b->hist[b->cur], 0, hist_bytes(b)));
    TSD_HIP(hipStreamSynchronize(nullptr));      // see tsdgpu_sos_reset
  }
  return TSDGPU_OK;
}

int tsdgpu_polyfir_bank_history_len(const tsdgpu_polyfir_bank *b) { return b ? b->HW : -1; }

int tsdgpu_polyfir_bank_get_state(tsdgpu_polyfir_bank *b, void *hist_dst, int *phase, void *stream)
{
  TSD_CHECK(b != nullptr, "polyfir_bank_get_state: NULL handle");
  TSD_CHECK(b->HW == 0 || hist_dst != nullptr, "polyfir_bank_get_state: NULL history buffer");
  if (phase) *phase = b->cnt;
  if (!b->HW) return TSDGPU_OK;
  hipStream_t st = (hipStream_t) stream;
  const bool dev = is_device_ptr(hist_dst);
  TSD_HIP(hipMemcpyAsync(hist_dst, b->hist[b->cur], hist_bytes(b), dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  if (!dev) TSD_HIP(hipStreamSynchronize(st));
  return TSDGPU_OK;
}

int tsdgpu_polyfir_bank_set_state(tsdgpu_polyfir_bank *b, const void *hist_src, int phase, void *stream)
{
  TSD_CHECK(b != nullptr, "polyfir_bank_set_state: NULL handle");
  TSD_CHECK(phase >= 0 && phase < b->R, "polyfir_bank_set_state: phase %d outside [0, %d)", phase, b->R);
  TSD_CHECK(b->HW == 0 || hist_src != nullptr, "polyfir_bank_set_state: NULL history buffer");
  b->cnt = phase;
  if (!b->HW) return TSDGPU_OK;
  hipStream_t st = (hipStream_t) stream;
  const bool dev = is_device_ptr(hist_src);
  TSD_HIP(hipMemcpyAsync(b->hist[b->cur], hist_src, hist_bytes(b), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  if (!dev) TSD_HIP(hipStreamSynchronize(st));   // (`hist_src` may die with the caller's scope)
  return TSDGPU_OK;
}

int tsdgpu_polyfir_bank_destroy(tsdgpu_polyfir_bank *b)
{
  if (!b) return TSDGPU_OK;
  if (b->d_g) (void) hipFree(b->d_g);
  if (b->hist[0]) (void) hipFree(b->hist[0]);   // (both histories live in the same allocation)
  b->in_stage.release();
  b->out_stage.release();
  delete b;
  return TSDGPU_OK;
}

}  // extern "C"
