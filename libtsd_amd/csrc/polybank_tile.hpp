// polybank_tile.hpp -- the device side the eight polyphase banks share (channelizer{,_os,_real,_real_os}.hip and
// synthesizer{,_os,_real,_real_os}.hip): a workgroup of CHAN_NT threads, R = CHAN_NT / T sub-runs of 16-frame units (T the
// transform length: M, or M / 2 in the real banks), one LDS image of 16 R frames at pitch FP (channelizer_internal.hpp).  Here are
// the thread's place in that tile, the channel-major read-back of the analysis banks, the real banks' untangling
// (channelizer_real{,_os}.hip) and tangling (synthesizer_real{,_os}.hip) steps with the pair load and store of their float stream,
// and the register window of a position with its fma chains.  Where a bank's samples come from and where its frames go stays in
// its own file, and so does the in-LDS transform of the tile (the R0 == 0 / s16::transform block): the files are built with
// -ffp-contract=fast, and behind a function the twiddle products of that block fuse differently and give other bits.
#pragma once
#include "channelizer_internal.hpp"
#include "stockham16.hpp"

namespace tsdgpu {

// Thread t: position s of sub-run r of R (NPOS = 2, M = 1024: one sub-run, the positions s and s + CHAN_NT); u0 the first unit of
// the sub-run, `per` units to a sub-run.
struct SubRun {
  int s, r, R;
  int64_t u0;
};
template <int NPOS> __device__ __forceinline__ SubRun sub_run(int t, int M, int lgM, int64_t per)
{
  const int s = NPOS == 1 ? t & (M - 1) : t, r = NPOS == 1 ? t >> lgM : 0, R = NPOS == 1 ? CHAN_NT >> lgM : 1;
  return {s, r, R, ((int64_t) blockIdx.x * R + r) * per};
}

// Item e of a channel-major pass over the tile of iteration `it`: (k, c, rr) = frames 2k, 2k + 1 of sub-run rr's unit, channel c;
// f the first of the two, counted in the step (negative in the synthesizer's unit it = -1).  8 lanes per 128-B segment.
struct TileItem {
  int k, c, rr;
  int64_t f;
};
__device__ __forceinline__ TileItem tile_item(int e, int M, int lgM, int R, int64_t per, int64_t it)
{
  const int k = e & 7, c = (e >> 3) & (M - 1), rr = e >> (3 + lgM);
  const int64_t un = ((int64_t) blockIdx.x * R + rr) * per + it;
  return {k, c, rr, (un << 4) + 2 * k};
}

// channel-major read-back of the transformed tile into the rows y + c ldy: a (channel, sub-run) pair receives its 16 frames as
// one 128-B segment, 16 B a lane where the rows are 16-B aligned (al), 2 x 8 B where not; frames from F on are not stored
template <int NPOS>
__device__ __forceinline__ void store_rows(const cpx *img, cpx *__restrict__ y, int64_t ldy, int M, int lgM, int FP, int64_t F,
                                           int64_t per, int64_t it, int R, int al, int t)
{
#pragma unroll 4
  for (int u = 0; u < 8 * NPOS; u++) {
    const TileItem q = tile_item(t + CHAN_NT * u, M, lgM, R, per, it);
    const cpx *src = img + (q.rr * 16 + 2 * q.k) * FP + s16::pad(q.c);
    const cpx a = src[0], b = src[FP];
    cpx *yc = y + (int64_t) q.c * ldy + q.f;
    if (q.f + 1 < F) {
      if (al) *reinterpret_cast<float4 *>(yc) = make_float4(a.x, a.y, b.x, b.y);
      else { yc[0] = a; yc[1] = b; }
    } else if (q.f < F) {
      yc[0] = a;
    }
  }
}

// Row c < N of a real frame of M = 2 N samples from the N-point transform Z of its even / odd packing (channelizer_real.hip):
// a = Z[c], b = Z[(N - c) mod N], w = W_M^c:  E = (a + conj b) / 2, O = (a - conj b) / (2 i), y_c = E + w O.
// At c = 0 (a = b, w = 1) the imaginary part comes out as 0 exactly.
__device__ __forceinline__ cpx untangle(cpx a, cpx b, cpx w)
{
  const float er = 0.5f * (a.x + b.x), ei = 0.5f * (a.y - b.y);
  const float orr = 0.5f * (a.y + b.y), oi = -0.5f * (a.x - b.x);
  return make_float2(er + (w.x * orr - w.y * oi), ei + (w.x * oi + w.y * orr));
}

// store_rows for the real-input bank: the image holds Z = DFT_N per frame; rows c < N are untangled on the way out, a
// (row, sub-run) pair still one 128-B segment; then row N, the Nyquist row Re Z[0] - Im Z[0], in a pass of 8 lanes per sub-run.
__device__ __forceinline__ void store_rows_real(const cpx *img, cpx *__restrict__ y, int64_t ldy, const cpx *__restrict__ WM, int N,
                                                int lgN, int FP, int64_t F, int64_t per, int64_t it, int R, int al, int t)
{
#pragma unroll 4
  for (int u = 0; u < 8; u++) {
    const TileItem q = tile_item(t + CHAN_NT * u, N, lgN, R, per, it);
    const cpx *fr = img + (q.rr * 16 + 2 * q.k) * FP;
    const int c0 = s16::pad(q.c), c1 = s16::pad((N - q.c) & (N - 1));
    const cpx w = WM[q.c];
    const cpx a = untangle(fr[c0], fr[c1], w), b = untangle(fr[FP + c0], fr[FP + c1], w);
    cpx *yc = y + (int64_t) q.c * ldy + q.f;
    if (q.f + 1 < F) {
      if (al) *reinterpret_cast<float4 *>(yc) = make_float4(a.x, a.y, b.x, b.y);
      else { yc[0] = a; yc[1] = b; }
    } else if (q.f < F) {
      yc[0] = a;
    }
  }
  if (t < 8 * R) {
    const TileItem q = tile_item(t, 1, 0, R, per, it);     // (k, rr) = (t & 7, t >> 3)
    const cpx *fr = img + (q.rr * 16 + 2 * q.k) * FP;
    const cpx z0 = fr[0], z1 = fr[FP];
    const cpx a = make_float2(z0.x - z0.y, 0.f), b = make_float2(z1.x - z1.y, 0.f);
    cpx *yc = y + (int64_t) N * ldy + q.f;
    if (q.f + 1 < F) {
      if (al) *reinterpret_cast<float4 *>(yc) = make_float4(a.x, a.y, b.x, b.y);
      else { yc[0] = a; yc[1] = b; }
    } else if (q.f < F) {
      yc[0] = a;
    }
  }
}

// untangle backwards, for the real-output synthesizer (synthesizer_real.hip): from the rows a = U_c, b = U_{N-c}, 0 < c < N / 2,
// and w = W_M^c the two inputs of the N-point inverse transform,
//   Z_c = A + T,  Z_{N-c} = conj A - conj T,   A = a + conj b,  T = i conj(w) (a - conj b)
// (W_M^{N-c} = -conj w), written to zc, zn with re and im swapped: the forward transform then serves as the inverse.
__device__ __forceinline__ void tangle_store(cpx *zc, cpx *zn, cpx a, cpx b, cpx w)
{
  const float ar = a.x + b.x, ai = a.y - b.y;
  const float dr = a.x - b.x, di = a.y + b.y;
  const float tr = w.y * dr - w.x * di, ti = w.x * dr + w.y * di;
  *zc = make_float2(ai + ti, ar + tr);
  *zn = make_float2(ti - ai, ar - tr);
}

// the lone pairs of that pass, swapped alike.  Z_0 = (Re U_0 + Re U_N) + i (Re U_0 - Re U_N): the imaginary parts of the rows 0
// and N are not used.  Z_{N/2} = 2 conj U_{N/2} (W_M^{N/2} = -i).
__device__ __forceinline__ cpx tangle_edge(cpx u0, cpx un) { return make_float2(u0.x - un.x, u0.x + un.x); }
__device__ __forceinline__ cpx tangle_mid(cpx um) { return make_float2(-2.f * um.y, 2.f * um.x); }

// two neighbouring real samples of a float stream as one complex position: one 8-B load where the stream is 8-B aligned (xal), two
// 4-B loads where not; and the store alike
__device__ __forceinline__ cpx load_pair(const float *__restrict__ p, int xal)
{
  return xal ? *reinterpret_cast<const cpx *>(p) : make_float2(p[0], p[1]);
}
__device__ __forceinline__ void store_pair(float *__restrict__ p, cpx v, int xal)
{
  if (xal) *reinterpret_cast<cpx *>(p) = v;
  else { p[0] = v.x; p[1] = v.y; }
}

// The register window of a position: cur[8] its values in the 8 frames of a half unit, prev[PW] those of the PW = (PP - 1) OS
// frames before, oldest first (OS = 1 where frames do not overlap).  Frame i of the half:
//   sum_{p = PP-1 .. 0} g[p] frame(i - p OS), frame(k) = cur[k] (k >= 0) or prev[PW + k]: oldest sample first
template <int PP, int OS>
__device__ __forceinline__ cpx window_chain(const float (&g)[PP], const cpx (&prev)[PP > 1 ? (PP - 1) * OS : 1], const cpx (&cur)[8], int i)
{
  constexpr int PW = (PP - 1) * OS;
  float ar = 0.f, ai = 0.f;
#pragma unroll
  for (int p = PP - 1; p >= 0; p--) {
    const int k = i - p * OS;
    const cpx w = k >= 0 ? cur[k >= 0 ? k : 0] : prev[k < 0 ? PW + k : 0];
    ar = fmaf(g[p], w.x, ar);
    ai = fmaf(g[p], w.y, ai);
  }
  return make_float2(ar, ai);
}

// The same chain for a position that holds two real samples (.x, .y) with a tap set each: g[p].x on the .x lane, g[p].y on the
// .y lane (the four real banks; OS > 1 in channelizer_real_os.hip alone, where the position's pairs lie D apart and the chain takes
// every OS-th).  Not one template with window_chain over the tap type: that reorders channelizer_real's instructions.
template <int PP, int OS>
__device__ __forceinline__ cpx window_chain_pair(const cpx (&g)[PP], const cpx (&prev)[PP > 1 ? (PP - 1) * OS : 1], const cpx (&cur)[8], int i)
{
  constexpr int PW = (PP - 1) * OS;
  float ar = 0.f, ai = 0.f;
#pragma unroll
  for (int p = PP - 1; p >= 0; p--) {
    const int k = i - p * OS;
    const cpx w = k >= 0 ? cur[k >= 0 ? k : 0] : prev[k < 0 ? PW + k : 0];
    ar = fmaf(g[p].x, w.x, ar);
    ai = fmaf(g[p].y, w.y, ai);
  }
  return make_float2(ar, ai);
}

// the window moves on by the half unit: prev = the last PW of (prev ++ cur)
template <int PW> __device__ __forceinline__ void window_shift(cpx (&prev)[PW > 0 ? PW : 1], const cpx (&cur)[8])
{
#pragma unroll
  for (int k = 0; k < PW; k++) prev[k] = k + 8 < PW ? prev[k + 8 < PW ? k + 8 : 0] : cur[k + 8 >= PW ? k + 8 - PW : 0];
}

}  // namespace tsdgpu
