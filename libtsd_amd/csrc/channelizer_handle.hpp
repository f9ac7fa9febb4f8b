// channelizer_handle.hpp -- the channelizer's handle, shared by its two kernel families: the maximally decimated bank
// (channelizer.hip) and the oversampled one (channelizer_os.hip).
#pragma once
#include "polybank_host.hpp"

// d_tab: g[p][s] = h[p M + M - 1 - s]; HW = P M - D ((P - 1) M at OS = 1) samples of the stream, oldest first
struct tsdgpu_channelizer : tsdgpu::PolyBank {
  int OS = 1, D = 0;                    // oversampling and hop D = M / OS: a step of n samples makes n / D frames
  int phase = 0;                        // hops consumed so far, modulo OS (host side; a launch argument)
};

namespace tsdgpu {

// channelizer_os.hip: one launch of the oversampled kernel (c->OS in {2, 4}) over F frames of hop c->D; reads c->phase
int chan_os_launch(tsdgpu_channelizer *c, const cpx *x, cpx *y, int64_t ldy, int64_t F, hipStream_t st);

}  // namespace tsdgpu
