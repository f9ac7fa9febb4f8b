// polybank_host.hpp -- the host side the polyphase banks share (channelizer.hip, channelizer_os.hip, synthesizer.hip,
// synthesizer_os.hip): what a
// handle holds, its tables and history, the geometry of a launch, and the map from M to the kernels' <R0, NPOS>.  The entry
// points, their argument checks and their messages stay with each operator.
#pragma once
#include "common.hpp"
#include "channelizer_internal.hpp"
#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

namespace tsdgpu {

using cpx = float2;

// What tsdgpu_channelizer and tsdgpu_synthesizer have in common.
struct PolyBank {
  int M = 0, lgM = 0, K = 0, P = 0;
  int HW = 0;                           // history samples (the operator says how many, and in which order)
  int hist_elem = sizeof(float2);       // bytes of a history sample: complex; float in the real-input channelizer
  int FP = 0;                           // pitch of a frame in the LDS image (samples)
  int cus = 0;
  float *d_tab = nullptr;               // the taps as P rows of M, then the twiddles W_M^i, i < M / 16 (one allocation)
  cpx *d_tw = nullptr;
  cpx *d_tw2 = nullptr;                 // real-input channelizer: W_M^c, c <= M / 2, behind the twiddles (which are W_{M/2}^i there)
  void *hist[2] = {nullptr, nullptr};   // HW samples (double-buffered, one allocation)
  int cur = 0;
  bool attr_set = false;                // the kernel of this shape may take its LDS
  DevBuf in_stage, out_stage;
};

inline size_t hist_bytes(const PolyBank *c) { return (size_t) c->HW * (size_t) c->hist_elem; }

// Fills a new handle: the shape (P = `rows` tap rows of M; 0: ceil(K / M)), the device's CUs, then one allocation and one upload: the P M taps, row p
// position s taking h[tap_index(p, s)] (zeros past K), then W_M^i, i < M / 16; and the zeroed double history of hist_len(P)
// samples.  `who` heads the messages.  On an error the caller destroys the handle.
// `half` = M / 2 (0: none) is the real-input channelizer's transform length: the frame pitch and the twiddles W_half^i, i < half / 16,
// are those of a half-point transform, and the untangling table W_M^c, c <= half, follows them.
template <typename HIST, typename INDEX>
int polybank_init(PolyBank *c, const char *who, int M, const float *taps_host, int ntaps, HIST hist_len, INDEX tap_index, int rows = 0,
                  int half = 0)
{
  c->M = M;
  c->lgM = __builtin_ctz((unsigned) M);
  c->K = ntaps;
  c->P = rows ? rows : (ntaps + M - 1) / M;
  c->HW = hist_len(c->P);
  const int T = half ? half : M;        // the transform length
  c->FP = chan_frame_pitch(T);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c->cus < 1)
    return set_err(TSDGPU_ERR_HIP, "%s: no device: %s", who, hipGetErrorString(hipGetLastError()));
  const size_t ng = (size_t) c->P * M, ntw = (size_t) std::max(T / 16, 1), nun = half ? (size_t) half + 1 : 0;
  std::vector<float> image(ng + 2 * ntw + 2 * nun, 0.f);
  for (int p = 0; p < c->P; p++)
    for (int s = 0; s < M; s++) {
      const int k = tap_index(p, s);
      image[(size_t) p * M + s] = k < ntaps ? taps_host[k] : 0.f;
    }
  const double PI = 3.14159265358979323846;
  for (size_t i = 0; i < ntw; i++) {
    const double a = -2.0 * PI * (double) i / (double) T;
    image[ng + 2 * i] = (float) std::cos(a);
    image[ng + 2 * i + 1] = (float) std::sin(a);
  }
  for (size_t i = 0; i < nun; i++) {
    const double a = -2.0 * PI * (double) i / (double) M;
    image[ng + 2 * (ntw + i)] = (float) std::cos(a);
    image[ng + 2 * (ntw + i) + 1] = (float) std::sin(a);
  }
  const size_t ib = image.size() * sizeof(float), hb = (hist_bytes(c) + 15) / 16 * 16;
  if (hipMalloc((void **) &c->d_tab, ib) != hipSuccess || (hb && hipMalloc(&c->hist[0], 2 * hb) != hipSuccess))
    return set_err(TSDGPU_ERR_ALLOC, "%s: hipMalloc of %zu bytes failed: %s", who, ib + 2 * hb, hipGetErrorString(hipGetLastError()));
  c->d_tw = reinterpret_cast<cpx *>(c->d_tab + ng);     // (ng is a multiple of 8: 8-B aligned)
  if (half) c->d_tw2 = c->d_tw + ntw;
  if (hb) c->hist[1] = (char *) c->hist[0] + hb;
  if (hipMemcpy(c->d_tab, image.data(), ib, hipMemcpyHostToDevice) != hipSuccess || (hb && hipMemset(c->hist[0], 0, 2 * hb) != hipSuccess) ||
      hipStreamSynchronize(nullptr) != hipSuccess)
    return set_err(TSDGPU_ERR_HIP, "%s: upload failed: %s", who, hipGetErrorString(hipGetLastError()));
  return TSDGPU_OK;
}

// A launch over F frames: `per` 16-frame units to each of a workgroup's sub-runs, two workgroups to a CU where one holds one
// position per thread (NPOS = 1).
struct PolyLaunch {
  int grid;
  int64_t per;
  size_t lds;
};
inline PolyLaunch polybank_geometry(int cus, int M, int lgM, int FP, int NPOS, int64_t F)
{
  const int R = NPOS == 1 ? CHAN_NT >> lgM : 1;
  const int64_t U = cdiv(F, 16);
  const int grid = (int) std::min<int64_t>((int64_t) cus * (NPOS == 1 ? 2 : 1), cdiv(U, R));
  return {grid, cdiv(U, (int64_t) grid * R), chan_lds_bytes(CHAN_NT * NPOS, M, FP)};
}
inline PolyLaunch polybank_geometry(const PolyBank *c, int NPOS, int64_t F) { return polybank_geometry(c->cus, c->M, c->lgM, c->FP, NPOS, F); }

// the rows of a step take 16-B loads and stores
inline int rows_aligned(const void *rows, int64_t ld) { return ((uintptr_t) rows & 15) == 0 && (ld & 1) == 0; }

// A handle launches one instantiation: it is asked once whether it may take its LDS, and a refusal is reported here, as `op`_step's,
// not as a failed launch.
inline int polybank_lds_attr(PolyBank *c, const void *kernel, const char *op, size_t lds)
{
  if (c->attr_set) return TSDGPU_OK;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e != hipSuccess) {
    (void) hipGetLastError();
    return set_err(TSDGPU_ERR_HIP, "%s_step: the kernel may not take its %zu bytes of LDS: %s", op, lds, hipGetErrorString(e));
  }
  c->attr_set = true;
  return TSDGPU_OK;
}

// fn(R0, NPOS) as std::integral_constants: R0 the first radix of the M-point transform (0: M = 8), NPOS = 2 at M = 1024
template <int V> using int_c = std::integral_constant<int, V>;
template <typename FN> int polybank_radix(int M, FN fn)
{
  switch (chan_radix0(M)) {
    case 0: return fn(int_c<0>(), int_c<1>());
    case 2: return fn(int_c<2>(), int_c<1>());
    case 4: return M == 1024 ? fn(int_c<4>(), int_c<2>()) : fn(int_c<4>(), int_c<1>());
    case 8: return fn(int_c<8>(), int_c<1>());
    default: return fn(int_c<16>(), int_c<1>());
  }
}

inline int polybank_reset(PolyBank *c)
{
  if (c->HW) {
    TSD_HIP(hipMemset(c->hist[c->cur], 0, hist_bytes(c)));
    TSD_HIP(hipStreamSynchronize(nullptr));      // see tsdgpu_sos_reset
  }
  return TSDGPU_OK;
}

// the current history to `dst` (get_state) or from `src` (set_state), whichever is given; a host buffer is waited for
inline int polybank_copy_state(PolyBank *c, void *dst, const void *src, hipStream_t st)
{
  if (!c->HW) return TSDGPU_OK;
  const bool dev = is_device_ptr(dst ? dst : src);
  if (dst) TSD_HIP(hipMemcpyAsync(dst, c->hist[c->cur], hist_bytes(c), dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  else TSD_HIP(hipMemcpyAsync(c->hist[c->cur], src, hist_bytes(c), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  if (!dev) TSD_HIP(hipStreamSynchronize(st));   // (`src` may die with the caller's scope)
  return TSDGPU_OK;
}

// what the handle holds on the device and in its staging buffers; the caller deletes the handle itself
inline void polybank_release(PolyBank *c)
{
  if (c->d_tab) (void) hipFree(c->d_tab);
  if (c->hist[0]) (void) hipFree(c->hist[0]);   // (both histories live in the same allocation)
  c->in_stage.release();
  c->out_stage.release();
}

}  // namespace tsdgpu
