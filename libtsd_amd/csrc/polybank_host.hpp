// polybank_host.hpp -- the host side the eight polyphase banks share (channelizer{,_os,_real,_real_os}.hip and
// synthesizer{,_os,_real,_real_os}.hip): the handle, the whole handle; the one create path with its argument checks and messages;
// the accessor bodies; the geometry of a launch and the launch itself; and the maps from M and P (or OS and P) to a kernel's
// template arguments.  The extern "C" entry points are in channelizer.hip and synthesizer.hip: a spec and a call, or a
// one-liner.  The other six files hold a kernel and its launch.
#pragma once
#include "common.hpp"
#include "channelizer_internal.hpp"
#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

namespace tsdgpu {

using cpx = float2;

// What a bank's handle holds.
// Analysis: d_tab g[p][s] = h[p M + M - 1 - s], P = ceil(K / M) rows; HW = P M - D samples of the stream, oldest first (floats in
// the real bank: hist_elem = 4).
// Synthesis: d_tab g[j][r] = f[j D + (r mod D)], P = ceil(K / D) rows; HW = (P - 1) rows samples as a (rows, P - 1) block: row c
// channel c's last P - 1 inputs, oldest first.
struct PolyBank {
  int M = 0, lgM = 0, K = 0, P = 0;
  int T = 0, lgT = 0;                   // the transform length: M; M / 2 in the real banks
  int OS = 1, D = 0;                    // oversampling and hop D = M / OS: a frame per D samples of the stream
  int phase = 0;                        // hops consumed so far, modulo OS (host side; a launch argument)
  bool real = false;                    // a float32 stream and M / 2 + 1 rows
  int HW = 0;                           // history samples
  int hist_elem = sizeof(float2);       // bytes of a history sample
  int FP = 0;                           // pitch of a frame in the LDS image (samples)
  int cus = 0;
  float *d_tab = nullptr;               // the taps as P rows of M, then the twiddles W_T^i, i < T / 16 (one allocation)
  cpx *d_tw = nullptr;
  cpx *d_tw2 = nullptr;                 // real banks: W_M^c, c <= M / 2, behind the twiddles
  void *hist[2] = {nullptr, nullptr};   // HW samples (double-buffered, one allocation)
  int cur = 0;
  bool attr_set = false;                // the kernel of this shape may take its LDS
  DevBuf in_stage, out_stage;
};

}  // namespace tsdgpu

// the C ABI's two opaque types: distinct, so that their pointers do not mix, and nothing but a PolyBank
struct tsdgpu_channelizer : tsdgpu::PolyBank {};
struct tsdgpu_synthesizer : tsdgpu::PolyBank {};

namespace tsdgpu {

// One launch over F frames of hop c->D, from the file named; the oversampled ones read c->phase.  x is a float stream in the
// real banks, which have M / 2 + 1 rows.
int chan_os_launch(tsdgpu_channelizer *c, const cpx *x, cpx *y, int64_t ldy, int64_t F, hipStream_t st);             // channelizer_os.hip
int chan_real_launch(tsdgpu_channelizer *c, const float *x, cpx *y, int64_t ldy, int64_t F, hipStream_t st);         // channelizer_real.hip
int chan_real_os_launch(tsdgpu_channelizer *c, const float *x, cpx *y, int64_t ldy, int64_t F, hipStream_t st);      // channelizer_real_os.hip
int syn_os_launch(tsdgpu_synthesizer *c, const cpx *u, int64_t ldu, cpx *x, int64_t F, hipStream_t st);              // synthesizer_os.hip
int syn_real_launch(tsdgpu_synthesizer *c, const cpx *u, int64_t ldu, float *x, int64_t F, hipStream_t st);          // synthesizer_real.hip
int syn_real_os_launch(tsdgpu_synthesizer *c, const cpx *u, int64_t ldu, float *x, int64_t F, hipStream_t st);       // synthesizer_real_os.hip

inline size_t hist_bytes(const PolyBank *c) { return (size_t) c->HW * (size_t) c->hist_elem; }

// rows a step writes (analysis) or reads (synthesis)
inline int polybank_rows(const PolyBank *c) { return c->real ? c->M / 2 + 1 : c->M; }

// What tells one create entry from another.
struct PolySpec {
  const char *who;                      // heads the messages
  bool synthesis;                       // the table, P and the history are the synthesis bank's (PolyBank above)
  bool real;
  int min_M;                            // the smallest M served
  const char *only_os1;                 // the entry serves OS = 1 alone and refuses the others with this text; nullptr: 1, 2 and 4
  bool per_channel;                     // at OS = 1 the tap limit is worded per channel, not per hop sample
  const PolySpec *at_one;               // OS = 1 is that entry's bank, made by it once the checks here have passed
};

// Fills a new handle of shape (M, OS): the device's CUs, then one allocation and one upload: the P rows of M taps (zeros past K),
// then W_T^i, i < T / 16, then in the real banks the (un)tangling table W_M^c, c <= M / 2; and the zeroed double history.
// On an error the caller releases the handle.
inline int polybank_init(PolyBank *c, const PolySpec &spec, int M, int OS, const float *taps_host, int ntaps)
{
  const int D = M / OS, T = spec.real ? M / 2 : M;
  c->M = M;
  c->lgM = __builtin_ctz((unsigned) M);
  c->T = T;
  c->lgT = __builtin_ctz((unsigned) T);
  c->OS = OS;
  c->D = D;
  c->real = spec.real;
  c->K = ntaps;
  c->P = spec.synthesis ? (ntaps + D - 1) / D : (ntaps + M - 1) / M;
  c->HW = spec.synthesis ? (c->P - 1) * polybank_rows(c) : c->P * M - D;
  c->hist_elem = spec.real && !spec.synthesis ? sizeof(float) : sizeof(cpx);
  c->FP = chan_frame_pitch(T);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c->cus < 1)
    return set_err(TSDGPU_ERR_HIP, "%s: no device: %s", spec.who, hipGetErrorString(hipGetLastError()));
  const size_t ng = (size_t) c->P * M, ntw = (size_t) std::max(T / 16, 1), nun = spec.real ? (size_t) T + 1 : 0;
  std::vector<float> image(ng + 2 * ntw + 2 * nun, 0.f);
  for (int p = 0; p < c->P; p++)
    for (int s = 0; s < M; s++) {
      const int k = spec.synthesis ? p * D + s % D : p * M + M - 1 - s;
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
    return set_err(TSDGPU_ERR_ALLOC, "%s: hipMalloc of %zu bytes failed: %s", spec.who, ib + 2 * hb, hipGetErrorString(hipGetLastError()));
  c->d_tw = reinterpret_cast<cpx *>(c->d_tab + ng);     // (ng is a multiple of 8: 8-B aligned)
  if (spec.real) c->d_tw2 = c->d_tw + ntw;
  if (hb) c->hist[1] = (char *) c->hist[0] + hb;
  if (hipMemcpy(c->d_tab, image.data(), ib, hipMemcpyHostToDevice) != hipSuccess || (hb && hipMemset(c->hist[0], 0, 2 * hb) != hipSuccess) ||
      hipStreamSynchronize(nullptr) != hipSuccess)
    return set_err(TSDGPU_ERR_HIP, "%s: upload failed: %s", spec.who, hipGetErrorString(hipGetLastError()));
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

template <typename HANDLE> int polybank_destroy(HANDLE *c)
{
  if (!c) return TSDGPU_OK;
  polybank_release(c);
  delete c;
  return TSDGPU_OK;
}

// The create entries: the checks in the order and the words of the C ABI, then the handle.
template <typename HANDLE>
int polybank_create(HANDLE **out, const PolySpec &spec, int channels, int oversample, const float *taps_host, int ntaps)
{
  const char *who = spec.who;
  TSD_CHECK(out != nullptr, "%s: out is NULL", who);
  *out = nullptr;
  TSD_CHECK(channels >= 1, "%s: channels = %d, need at least one", who, channels);
  TSD_CHECK(oversample >= 1, "%s: oversample = %d, need at least one", who, oversample);
  TSD_CHECK(taps_host != nullptr && ntaps >= 1, "%s: K > 0 taps required", who);
  if (!chan_served_channels(channels, spec.min_M))
    return set_err(TSDGPU_ERR_UNSUPPORTED, "%s: channels = %d: served are the powers of two from %d to %d", who, channels, spec.min_M, CHAN_MAX_M);
  if (spec.only_os1 ? oversample != 1 : !chan_served_oversample(oversample))
    return set_err(TSDGPU_ERR_UNSUPPORTED, "%s: oversample = %d: %s", who, oversample, spec.only_os1 ? spec.only_os1 : "served are 1, 2 and 4");
  // K <= 16 D: P OS <= 16 (synthesis: Q <= 16), the register window of a position stays within 15 older samples
  const int hop = channels / oversample;
  if (spec.per_channel && oversample == 1 && ntaps > CHAN_MAX_P * channels)
    return set_err(TSDGPU_ERR_UNSUPPORTED, "%s: %d taps over %d channels: served are up to %d taps per channel (%d taps)", who, ntaps, channels,
                   CHAN_MAX_P, CHAN_MAX_P * channels);
  if (ntaps > CHAN_MAX_P * hop)
    return set_err(TSDGPU_ERR_UNSUPPORTED, "%s: %d taps over %d channels at hop %d: served are up to %d taps per hop sample (%d taps)", who, ntaps,
                   channels, hop, CHAN_MAX_P, CHAN_MAX_P * hop);
  // (the maximally decimated real bank: its own entry, kernel and bits)
  if (oversample == 1 && spec.at_one) return polybank_create(out, *spec.at_one, channels, 1, taps_host, ntaps);
  HANDLE *c = new HANDLE();
  if (const int rc = polybank_init(c, spec, channels, oversample, taps_host, ntaps)) {
    polybank_destroy(c);
    return rc;
  }
  *out = c;
  return TSDGPU_OK;
}

// The accessor bodies; `op` ("channelizer", "synthesizer") or `fn` (the entry's name) heads the message.
inline int polybank_hop(const PolyBank *c) { return c ? c->D : -1; }
inline int polybank_history_len(const PolyBank *c) { return c ? c->HW : -1; }
inline int polybank_get_phase(const PolyBank *c) { return c ? c->phase : -1; }
inline int polybank_rows_of(const PolyBank *c) { return c ? polybank_rows(c) : -1; }
inline int polybank_is_real(const PolyBank *c) { return c ? (int) c->real : -1; }

inline int polybank_set_phase(PolyBank *c, const char *op, int64_t hops)
{
  TSD_CHECK(c != nullptr, "%s_set_phase: NULL handle", op);
  TSD_CHECK(hops >= 0, "%s_set_phase: %lld hops, a negative count", op, (long long) hops);
  c->phase = (int) (hops % c->OS);
  return TSDGPU_OK;
}

inline int polybank_reset(PolyBank *c, const char *op)
{
  TSD_CHECK(c != nullptr, "%s_reset: NULL handle", op);
  if (c->HW) {
    TSD_HIP(hipMemset(c->hist[c->cur], 0, hist_bytes(c)));
    TSD_HIP(hipStreamSynchronize(nullptr));      // see tsdgpu_sos_reset
  }
  c->phase = 0;
  return TSDGPU_OK;
}

// the current history to `dst` (get_state) or from `src` (set_state), whichever is given; a host buffer is waited for
inline int polybank_copy_state(PolyBank *c, const char *fn, void *dst, const void *src, hipStream_t st)
{
  TSD_CHECK(c != nullptr, "%s: NULL handle", fn);
  TSD_CHECK(c->HW == 0 || dst != nullptr || src != nullptr, "%s: NULL history buffer", fn);
  if (!c->HW) return TSDGPU_OK;
  const bool dev = is_device_ptr(dst ? dst : src);
  if (dst) TSD_HIP(hipMemcpyAsync(dst, c->hist[c->cur], hist_bytes(c), dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  else TSD_HIP(hipMemcpyAsync(c->hist[c->cur], src, hist_bytes(c), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  if (!dev) TSD_HIP(hipStreamSynchronize(st));   // (`src` may die with the caller's scope)
  return TSDGPU_OK;
}

// A launch over F frames: `per` 16-frame units to each of a workgroup's sub-runs, two workgroups to a CU where one holds one
// position per thread (NPOS = 1).
struct PolyLaunch {
  int grid;
  int64_t per;
  size_t lds;
};
inline PolyLaunch polybank_geometry(const PolyBank *c, int NPOS, int64_t F)
{
  const int R = NPOS == 1 ? CHAN_NT >> c->lgT : 1;
  const int64_t U = cdiv(F, 16);
  const int grid = (int) std::min<int64_t>((int64_t) c->cus * (NPOS == 1 ? 2 : 1), cdiv(U, R));
  return {grid, cdiv(U, (int64_t) grid * R), chan_lds_bytes(CHAN_NT * NPOS, c->T, c->FP)};
}

// the rows of a step take 16-B loads and stores; a float stream takes its pairs as 8 B
inline int rows_aligned(const void *rows, int64_t ld) { return ((uintptr_t) rows & 15) == 0 && (ld & 1) == 0; }
inline int stream_aligned(const void *x) { return ((uintptr_t) x & 7) == 0; }

// `kernel`(args...) over the geometry g.  A handle launches one instantiation: it is asked once whether it may take its LDS, and
// a refusal is reported here, as `op`_step's, not as a failed launch.
template <typename... KA, typename... A>
int polybank_launch(PolyBank *c, const char *op, void (*kernel)(KA...), const PolyLaunch &g, hipStream_t st, A... args)
{
  if (!c->attr_set) {
    const hipError_t e = hipFuncSetAttribute((const void *) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) {
      (void) hipGetLastError();
      return set_err(TSDGPU_ERR_HIP, "%s_step: the kernel may not take its %zu bytes of LDS: %s", op, g.lds, hipGetErrorString(e));
    }
    c->attr_set = true;
  }
  hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(CHAN_NT), g.lds, st, args...);
  TSD_HIP(hipGetLastError());
  return TSDGPU_OK;
}

// The maps to a kernel's template arguments, as int_c of common.hpp.
constexpr int POLYBANK_UNSERVED = -1;   // no case below: the caller words the refusal (not a status of tsdgpu.h)

// fn(R0, NPOS): R0 the first radix of the T-point transform (0: T = 8), NPOS = 2 at T = 1024
template <typename FN> int polybank_radix(int T, FN fn)
{
  switch (chan_radix0(T)) {
    case 0: return fn(int_c<0>(), int_c<1>());
    case 2: return fn(int_c<2>(), int_c<1>());
    case 4: return T == 1024 ? fn(int_c<4>(), int_c<2>()) : fn(int_c<4>(), int_c<1>());
    case 8: return fn(int_c<8>(), int_c<1>());
    default: return fn(int_c<16>(), int_c<1>());
  }
}

// fn(P), P = 1 .. 16 tap rows
template <typename FN> int polybank_taps(int P, FN fn)
{
  switch (P) {
    case 1: return fn(int_c<1>());
    case 2: return fn(int_c<2>());
    case 3: return fn(int_c<3>());
    case 4: return fn(int_c<4>());
    case 5: return fn(int_c<5>());
    case 6: return fn(int_c<6>());
    case 7: return fn(int_c<7>());
    case 8: return fn(int_c<8>());
    case 9: return fn(int_c<9>());
    case 10: return fn(int_c<10>());
    case 11: return fn(int_c<11>());
    case 12: return fn(int_c<12>());
    case 13: return fn(int_c<13>());
    case 14: return fn(int_c<14>());
    case 15: return fn(int_c<15>());
    case 16: return fn(int_c<16>());
    default: return POLYBANK_UNSERVED;
  }
}

// fn(P, OS) where the oversampling is a template argument too (the analysis banks): P OS <= 16, OS in {2, 4}
template <typename FN> int polybank_os_taps(int OS, int P, FN fn)
{
  switch (OS * 100 + P) {
    case 201: return fn(int_c<1>(), int_c<2>());
    case 202: return fn(int_c<2>(), int_c<2>());
    case 203: return fn(int_c<3>(), int_c<2>());
    case 204: return fn(int_c<4>(), int_c<2>());
    case 205: return fn(int_c<5>(), int_c<2>());
    case 206: return fn(int_c<6>(), int_c<2>());
    case 207: return fn(int_c<7>(), int_c<2>());
    case 208: return fn(int_c<8>(), int_c<2>());
    case 401: return fn(int_c<1>(), int_c<4>());
    case 402: return fn(int_c<2>(), int_c<4>());
    case 403: return fn(int_c<3>(), int_c<4>());
    case 404: return fn(int_c<4>(), int_c<4>());
    default: return POLYBANK_UNSERVED;
  }
}

}  // namespace tsdgpu
