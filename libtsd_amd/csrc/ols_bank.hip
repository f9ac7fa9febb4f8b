// ols_bank.hip -- overlap-save FIR bank: long filters over C channels in one launch per step.
//
// The frequency-domain path of tsdgpu_fir_bank (bank.hip).  The block arithmetic is the single-stream plan's (ols.hip): N = 1024
// points on the in-wave transform of fft1024_wave.hpp, the overlap rounded up to whole 64-sample rows, L = 1024 - 64 ceil((K-1)/64)
// outputs per block, the response H and the two twiddle tables read from the image [H | tw1 | tw2] that ols_plan_create uploads
// behind the prototype handle's d_H.  What differs is the walk: a work unit is (channel c, block b) -- for real data the pair of
// blocks (2b, 2b+1) OF THE SAME CHANNEL, packed as real and imaginary part -- numbered channel-major with a 64-bit linear index
// (no grid.y, no chunking of the channel count), handed out statically (unit = wave + i * grid) to a persistent grid of one-wave
// workgroups.  Two channels never share a transform: the rounding error of a loud channel and a channel's non-finite samples
// stay inside that channel.
//
// Edges.  L and the overlap are multiples of 64, so every 64-sample input row of a block starts on a multiple of 64 relative to
// the channel's sample 0: a row lies wholly in the channel's history (before 0) or wholly at or after 0, and the choice between
// the two bases is a scalar one.  Only the row that straddles n has lanes to mask, and that is one compare per row against a
// scalar count (`rem`), not per-sample address arithmetic: all 16 row loads of every unit are issued unconditionally from valid
// addresses, in straight-line code, and the lanes past n are zeroed once the loads have landed.  In the shapes banks run at a
// large share of the units are first or last blocks of their channel: there is no separate slow edge path.
//
// The wave that owns a channel's last unit also writes the channel's new history row (the last HL samples of old history ++ x)
// into the other buffer of the bank's double-buffered C x HL array: no history kernel, no memset, one launch per step.
#include "fir_internal.hpp"
#include "bank_internal.hpp"
#include "fft1024_wave.hpp"
#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace tsdgpu {

using namespace w1024;
namespace {
constexpr int OB_N = 1024;
using cv = cpx;

struct RegTab {
  cv v[16];
  __device__ __forceinline__ const cv &operator[](int r) const { return v[r]; }
};

template <bool REAL>
__global__ __launch_bounds__(64, 2) void ols_bank_kernel(const void *__restrict__ xv, int64_t ldx, void *__restrict__ yv, int64_t ldy,
                                                         const cpx *__restrict__ tab, int ovl, int L, int64_t n, int64_t upc,
                                                         int64_t nunits, const void *__restrict__ hist_old,
                                                         void *__restrict__ hist_new, int HL)
{
  __shared__ cv lds[LDS_ELEMS];
  using S = typename std::conditional<REAL, float, cv>::type;      // a sample of the stream
  const int lane = threadIdx.x & 63;
  const S *x = (const S *) xv, *ho = (const S *) hist_old;
  S *y = (S *) yv, *hn = (S *) hist_new;
  RegTab tw1r, tw2r, Hr;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    Hr.v[r] = tab[r * 64 + lane];
    tw1r.v[r] = tab[OB_N + r * 64 + lane];
    tw2r.v[r] = tab[2 * OB_N + r * 64 + lane];
  }
  // one wave per workgroup: LDS operations execute in order, wave-scope fences only pin the compiler (ols.hip: ols_body)
  auto sync = []() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  const bool small = nunits <= 0x7fffffff;
  auto split = [&](int64_t u, int64_t &c, int64_t &b) {
    if (small) c = (int64_t) ((uint32_t) u / (uint32_t) upc);
    else c = u / upc;
    b = u - c * upc;
  };
  // One input block of a channel, as the scalars its 16 row loads need.  Position t = 64 r + lane of the block is sample
  // gs0 + t of the channel, gs0 = blk L - ovl a multiple of 64: rows below `hrows` lie wholly in the channel's history row
  // (read at pH + t), the others at or after sample 0 (read at pX + t), of which the positions from `rel` on lie past n and
  // are zeros.  A lane past n loads the last sample below it instead (position rel - 1), so every load is unconditional and
  // in bounds; a block wholly past n (the second of a real pair) loads the channel's sample 0.
  struct Blk {
    const S *pH, *pX;
    int hrows, rel, cap;
  };
  auto blk_of = [&](int64_t c, int64_t blk) -> Blk {
    Blk k;
    const int64_t gs0 = blk * (int64_t) L - ovl;
    const S *xc = x + c * ldx;
    const int64_t d = n - gs0;
    k.hrows = gs0 < 0 ? (int) ((-gs0) >> 6) : 0;
    k.rel = d <= 0 ? 0 : (d >= OB_N ? OB_N : (int) d);
    k.pH = ho + c * (int64_t) HL + (HL + gs0);
    k.pX = d <= 0 ? xc : xc + gs0;
    k.cap = k.rel > 0 ? k.rel - 1 : 0;
    return k;
  };
  auto row_ptr = [&](const Blk &k, int r) -> const S * {
    const int t = 64 * r + lane;
    return r < k.hrows ? k.pH + t : k.pX + (t < k.cap ? t : k.cap);
  };
  struct Unit {
    int64_t c, b;
    Blk k0, k1;      // (k1: the second block of a real pair)
  };
  auto unit_of = [&](int64_t u) -> Unit {
    Unit q;
    split(u, q.c, q.b);
    q.k0 = blk_of(q.c, REAL ? 2 * q.b : q.b);
    q.k1 = REAL ? blk_of(q.c, 2 * q.b + 1) : q.k0;
    return q;
  };
  // the 16 row loads of a unit ...
  auto fetch = [&](cv (&v)[16], const Unit &q) {
#pragma unroll
    for (int r = 0; r < 16; r++) {
      if (!REAL) v[r] = *(const cv *) row_ptr(q.k0, r);
      else v[r] = mk(*(const float *) row_ptr(q.k0, r), *(const float *) row_ptr(q.k1, r));
    }
  };
  // ... and the zero fill of what lies past n, once they have landed
  auto mask = [&](cv (&v)[16], const Unit &q) {
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int t = 64 * r + lane;
      if (!REAL) {
        if (r >= q.k0.hrows && t >= q.k0.rel) v[r] = mk(0.f, 0.f);
      } else {
        if (r >= q.k0.hrows && t >= q.k0.rel) v[r].x = 0.f;
        if (r >= q.k1.hrows && t >= q.k1.rel) v[r].y = 0.f;
      }
    }
  };

  const int64_t G = gridDim.x;
  int64_t unit = blockIdx.x;
  if (unit >= nunits) return;

  // One unit: prefetch unit `nu` into nxt, transform cur in place, wait for the prefetch (the youngest memory operations of the
  // wave: the stores of the unit before are older and had a whole transform to drain), then the channel's history if this is
  // its last unit, then the stores -- nothing waits on them, they drain under the next transform.
  auto process = [&](cv (&cur)[16], cv (&nxt)[16], int64_t u, int64_t nu) {
    {
      const Unit qn = unit_of(nu);
      fetch(nxt, qn);
      forward(cur, lds, lane, tw1r, tw2r, sync);
#pragma unroll
      for (int r = 0; r < 16; r++) cur[r] = cmul(cur[r], Hr[r]);
      inverse(cur, lds, lane, tw1r, tw2r, sync);
      sync();   // LDS is reused by the next unit
#pragma unroll
      for (int r = 0; r < 16; r++) asm volatile("" ::"v"(nxt[r]));
      mask(nxt, qn);
    }
    int64_t c, b;
    split(u, c, b);
    const S *xc = x + c * ldx;
    S *yc = y + c * ldy;
    if (b == upc - 1) {
      const S *oh = ho + c * (int64_t) HL;
      S *nh = hn + c * (int64_t) HL;
      for (int i = lane; i < HL; i += 64) {
        const int64_t g = n - HL + i;
        nh[i] = g < 0 ? oh[HL + g] : xc[g];
      }
    }
    // position t = 64 r + lane of the circular convolution is output o0 + t - ovl: positions below ovl are overlap, and the
    // outputs from n on do not exist
    auto out_rel = [&](int64_t o0) -> int {
      const int64_t d = n - (o0 - ovl);
      return d <= 0 ? 0 : (d >= OB_N ? OB_N : (int) d);
    };
    if (!REAL) {
      const int64_t o0 = b * (int64_t) L;
      cv *yb = (cv *) yc + (o0 - ovl);
      const int rel = out_rel(o0);
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int t = 64 * r + lane;
        if (t >= ovl && t < rel) yb[t] = cur[r];
      }
    } else {
      const int64_t oa = 2 * b * (int64_t) L, ob = oa + L;
      float *ya = (float *) yc + (oa - ovl), *yb = (float *) yc + (ob - ovl);
      const int rela = out_rel(oa), relb = out_rel(ob);
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int t = 64 * r + lane;
        if (t >= ovl && t < rela) ya[t] = cur[r].x;
        if (t >= ovl && t < relb) yb[t] = cur[r].y;
      }
    }
  };

  cv A[16], B[16];
  {
    const Unit q0 = unit_of(unit);
    fetch(A, q0);
  // (waited for before the loop, as in ols_body: left in flight into it, the loop head would merge "A in flight" with "A landed")
#pragma unroll
  for (int r = 0; r < 16; r++) asm volatile("" ::"v"(A[r]));
    mask(A, q0);
  }
  for (;;) {
    // a wave's last unit prefetches itself again (in bounds, an L2 hit), so that no path of the loop skips the loads
    int64_t nu = unit + G;
    bool more = nu < nunits;
    process(A, B, unit, more ? nu : unit);
    if (!more) break;
    unit = nu;
    nu = unit + G;
    more = nu < nunits;
    process(B, A, unit, more ? nu : unit);
    if (!more) break;
    unit = nu;
  }
}

}  // namespace

// The 1024-point plan on the bank's prototype handle, whatever the tap count inside the kernel's envelope (a single handle of
// 514 .. 961 taps would take the long-filter plan): fills d_H, ols_L; leaves the handle's own method alone.  *served: false
// when the tap count lies outside the envelope (K < 2 or K > 961) and the bank stays on the direct scheme.
int ols_bank_plan(tsdgpu_fir *proto, bool *served, int *grid)
{
  *served = false;
  *grid = 0;
  if (proto->K < 2 || proto->K > OB_N - 63) return TSDGPU_OK;
  const int method = proto->method;
  proto->ols_short_only = true;
  const int rc = ols_plan_create(proto);
  proto->method = method;
  if (rc) return rc;
  if (!proto->d_H) return TSDGPU_OK;
  // persistent grid: as many waves as the device keeps resident (asked once per process: the devices of a node are alike)
  static const int resident = []() {
    int dev = 0, cus = 256, per_cu = 8;
    (void) hipGetDevice(&dev);
    (void) hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, ols_bank_kernel<false>, 64, 0) != hipSuccess || per_cu < 1) {
      (void) hipGetLastError();
      per_cu = 8;
    }
    return cus * per_cu;
  }();
  *grid = resident;
  *served = true;
  return TSDGPU_OK;
}

int ols_bank_overlap(const tsdgpu_fir *proto) { return OB_N - proto->ols_L; }

// AUTO, per step, from (taps, types, n).  Both schemes timed at C * n = 2^24 samples, n = 64 .. 65536, in one process
// (profiles/r7_perf_ols_bank.txt; times in ms, direct / overlap-save):
//  - lower tap count.  Complex data, real taps: the single handle's 57 (K = 57: 0.124 / 0.104 at n = 512, 0.066 / 0.066 at
//    4096, 0.063 / 0.061 at 65536; only channels just longer than one block lose -- n = 1024: 0.086 / 0.101, still 0.098 /
//    0.100 at K = 96).  Real data: 97, not the single handle's 40 -- two real blocks share a transform but each 4-B row load
//    moves half the bytes of a complex one, and the direct bank's real kernel steps its cost at multiples of 32 taps: K = 57:
//    0.041 / 0.054 at n = 4096, K = 96: 0.048 / 0.054, K = 112 (the first multiple above): 0.056 / 0.054, and ahead at every n.
//    Complex taps: the single handle's 48 (not timed for the bank: the direct scheme pays twice the multiply-adds of real taps
//    there, overlap-save the same).
//  - upper tap count.  Up to 897 taps (L >= 128) overlap-save wins or ties at every n (K = 897, n = 4096: 0.295 / 0.268
//    real, 0.536 / 0.543 complex; K = 833: 0.275 / 0.153).  From 898 taps a block yields 64 outputs for 1024 points, and only
//    short channels, where the direct bank's 2048-sample tiles idle, still gain: K = 961, real data: 0.771 / 0.547 at n = 512
//    against 0.412 / 0.545 at 1024; complex: 1.597 / 1.247 at n = 256 against 0.871 / 1.213 at 512.
//  - no lower bound on n: the shorter the channels, the further ahead overlap-save is (K = 127, complex, n = 64: 1.046 / 0.719).
constexpr int OLS_BANK_K_FULL = 897;     // the last tap count with L >= 128
bool ols_bank_preferred(const tsdgpu_fir *proto, int64_t n)
{
  const int K = proto->K;
  const bool real = proto->data_type == TSDGPU_F32;
  const int k_lo = real ? 97 : (proto->tap_type == TSDGPU_F32 ? 57 : 48);
  if (!proto->d_H || K < k_lo) return false;
  if (K <= OLS_BANK_K_FULL) return true;
  return n <= (real ? 512 : 256);
}

int ols_bank_launch(const tsdgpu_fir *proto, int grid, int64_t C, const void *x, int64_t ldx, void *y, int64_t ldy, int64_t n,
                    const void *hist_old, void *hist_new, int HL, hipStream_t st)
{
  const bool real = proto->data_type == TSDGPU_F32;
  const int L = proto->ols_L;
  const int64_t upc = cdiv(n, real ? 2 * (int64_t) L : L);      // units per channel
  const int64_t nunits = upc * C;
  const unsigned g = (unsigned) std::min<int64_t>(nunits, grid);
  const cpx *tab = (const cpx *) proto->d_H;
  if (real)
    hipLaunchKernelGGL(ols_bank_kernel<true>, dim3(g), dim3(64), 0, st, x, ldx, y, ldy, tab, OB_N - L, L, n, upc, nunits, hist_old, hist_new, HL);
  else
    hipLaunchKernelGGL(ols_bank_kernel<false>, dim3(g), dim3(64), 0, st, x, ldx, y, ldy, tab, OB_N - L, L, n, upc, nunits, hist_old, hist_new, HL);
  if (const hipError_t le = hipGetLastError(); le != hipSuccess)
    return set_err(TSDGPU_ERR_HIP, "fir_bank_step: overlap-save launch failed: %s", hipGetErrorString(le));
  return TSDGPU_OK;
}

}  // namespace tsdgpu
