// channelizer_handle.hpp -- the channelizer's handle, shared by its four kernel families: the maximally decimated bank
// (channelizer.hip), the oversampled one (channelizer_os.hip), the real-input one (channelizer_real.hip) and the oversampled
// real-input one (channelizer_real_os.hip).
#pragma once
#include "polybank_host.hpp"

// d_tab: g[p][s] = h[p M + M - 1 - s]; HW = P M - D ((P - 1) M at OS = 1) samples of the stream, oldest first
struct tsdgpu_channelizer : tsdgpu::PolyBank {
  int OS = 1, D = 0;                    // oversampling and hop D = M / OS: a step of n samples makes n / D frames
  int phase = 0;                        // hops consumed so far, modulo OS (host side; a launch argument)
  bool real = false;                    // a float32 stream into M / 2 + 1 rows; the history is P M - D floats (hist_elem = 4)
};

namespace tsdgpu {

// channelizer_os.hip: one launch of the oversampled kernel (c->OS in {2, 4}) over F frames of hop c->D; reads c->phase
int chan_os_launch(tsdgpu_channelizer *c, const cpx *x, cpx *y, int64_t ldy, int64_t F, hipStream_t st);

// channelizer_real.hip: one launch of the real-input kernel (c->real) over F frames of M floats into M / 2 + 1 rows
int chan_real_launch(tsdgpu_channelizer *c, const float *x, cpx *y, int64_t ldy, int64_t F, hipStream_t st);

// channelizer_real_os.hip: one launch of the oversampled real-input kernel (c->real, c->OS in {2, 4}) over F frames of hop c->D
// floats into M / 2 + 1 rows; reads c->phase
int chan_real_os_launch(tsdgpu_channelizer *c, const float *x, cpx *y, int64_t ldy, int64_t F, hipStream_t st);

// rows a step writes
inline int chan_rows(const tsdgpu_channelizer *c) { return c->real ? c->M / 2 + 1 : c->M; }

}  // namespace tsdgpu
