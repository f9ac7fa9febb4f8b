// poly_internal.hpp -- host-side plan of the integer-rate FIR stages, shared by the single-stream handle (polyphase.hip) and
// the channel bank (rate_bank.hip): the tap image of a stage, the outputs per workgroup of the oldest-first scheme and the
// regime of the direct scheme.  Both translation units must build the SAME image and choose the SAME scheme: a bank channel
// is bit-identical to a single-stream handle because of it.
#pragma once
#include "common.hpp"
#include <algorithm>
#include <vector>

namespace tsdgpu {

#ifndef PF_SPAN_TARGET
#define PF_SPAN_TARGET 2048
#endif
constexpr int PF_TO = 2048;          // outputs per workgroup (fewer when the decimation rate makes their input span too long)
constexpr int PF_MAX_SPAN = 16000;   // staged input samples per workgroup (129 KiB of complex data with the padding)

// Output o of a stage belongs to group grp = o / NPH and phase ph = o % NPH and is
//     y[o] = sum_{k < W} g[ph][k] * x[grp * stride + start - k]          (x[i < 0] = history)
// Decimators: NPH = 1, stride = R.  Upsampler: NPH = R, stride = 1, one W = ceil(K/R)-tap branch per output phase.
struct PolyImage {
  std::vector<float> g;              // [NPH][W], FIR convention: g[ph][0] meets the newest sample
  int NPH = 1, W = 0, stride = 1;
};

// kind: TSDGPU_POLY_DECIM / _HALFBAND / _UPS (R already forced to 2 for the half-band)
inline PolyImage poly_tap_image(int kind, const float *taps_host, int ntaps, int R)
{
  PolyImage im;
  if (kind == TSDGPU_POLY_DECIM || kind == TSDGPU_POLY_HALFBAND) {
    // window is correlated with the taps in forward order (polyphase.cc:223-229) == an FIR
    // with the taps reversed; half-band keeps the even taps and forces 0.5 on the centre sample
    im.g.resize((size_t) ntaps);
    for (int k = 0; k < ntaps; k++) {
      const int i = ntaps - 1 - k;
      float c = taps_host[i];
      if (kind == TSDGPU_POLY_HALFBAND) c = ((i & 1) == 0 ? c : 0.f) + (i == ntaps / 2 ? 0.5f : 0.f);
      im.g[k] = c;
    }
    im.NPH = 1;
    im.W = ntaps;
    im.stride = R;
  } else {
    // coefs = c * R, zero-padded to a multiple of R (polyphase.cc:259-270); phase i correlates
    // the K/R-sample window with coefs[(R-1-i) + j*R]
    std::vector<float> c((size_t) ntaps);
    for (int i = 0; i < ntaps; i++) c[i] = taps_host[i] * (float) R;
    while (c.size() % (size_t) R) c.push_back(0.f);
    const int W = (int) c.size() / R;
    for (int i = 0; i < R; i++)
      for (int k = 0; k < W; k++) im.g.push_back(c[(size_t) (R - 1 - i) + (size_t) (W - 1 - k) * R]);
    im.NPH = R;
    im.W = W;
    im.stride = 1;
  }
  return im;
}

// outputs per workgroup of the oldest-first scheme: as many as keep the staged input span within PF_MAX_SPAN samples
// ... and preferably within ~PF_SPAN_TARGET samples (17 KiB: several workgroups per CU overlap their load and compute phases)
inline int64_t poly_fused_outputs(int NPH, int W, int stride)
{
  int64_t to = std::min<int64_t>(PF_TO, ((int64_t) (PF_MAX_SPAN - W) / stride - 1) * NPH);
  return std::min<int64_t>(to, std::max<int64_t>(256, (int64_t) (PF_SPAN_TARGET / stride) * NPH));
}
// the oldest-first scheme serves a stage when its taps and the input span of 256 outputs or more fit in LDS
inline bool poly_fused_serves(int NPH, int W, int stride) { return poly_fused_outputs(NPH, W, stride) >= 256 && (size_t) NPH * W <= 4096 && W >= 1; }

// the direct scheme: decimators of rate 2 / 4 / 8 up to 64 taps, upsamplers of rate 2 / 4 with branches of up to 32 taps
inline bool poly_direct_regime(int NPH, int W, int stride)
{
  const bool updir = stride == 1 && (NPH == 2 || NPH == 4) && W <= 32;
  return (NPH == 1 && (stride == 2 || stride == 4 || stride == 8) && W <= 64) || updir;
}
// the direct scheme's tap rows: KP = W rounded up to two lane segments (RS = 64 B of samples); hrev[i][j] = g[i][KP - 1 - j]
inline int poly_direct_kp(int W, int data_type)
{
  const int RSd = data_type == TSDGPU_F32 ? 16 : 8;
  return (int) (cdiv(W, 2 * RSd) * 2 * RSd);
}
inline void poly_direct_rows(const std::vector<float> &g, int NPH, int W, int KP, float *hr)
{
  for (int i = 0; i < NPH; i++)
    for (int k = 0; k < W; k++) hr[(size_t) i * KP + KP - 1 - k] = g[(size_t) i * W + k];   // g[0] meets the newest sample
}

}  // namespace tsdgpu
