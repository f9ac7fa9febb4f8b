// channelizer_handle.hpp -- the channelizer's handle, shared by its two kernel families: the maximally decimated bank
// (channelizer.hip) and the oversampled one (channelizer_os.hip).
#pragma once
#include "common.hpp"
#include "channelizer_internal.hpp"

namespace tsdgpu { using cpx = float2; }

struct tsdgpu_channelizer {
  int M = 0, lgM = 0, K = 0, P = 0;
  int OS = 1, D = 0;                    // oversampling and hop D = M / OS: a step of n samples makes n / D frames
  int phase = 0;                        // hops consumed so far, modulo OS (host side; a launch argument)
  int HW = 0;                           // history samples: P M - D ((P - 1) M at OS = 1)
  int FP = 0;                           // pitch of a frame in the LDS image (samples)
  int cus = 0;
  float *d_g = nullptr;                 // g[p][s], P rows of M, then the twiddles W_M^i, i < M / 16 (one allocation)
  tsdgpu::cpx *d_tw = nullptr;
  void *hist[2] = {nullptr, nullptr};   // HW samples, oldest first (double-buffered, one allocation)
  int cur = 0;
  bool attr_set = false;                // the kernel of this shape may take its LDS
  tsdgpu::DevBuf in_stage, out_stage;
};

namespace tsdgpu {

constexpr int CHAN_NT = 512;          // threads of a workgroup

// channelizer_os.hip: one launch of the oversampled kernel (c->OS in {2, 4}) over F frames of hop c->D; reads c->phase
int chan_os_launch(tsdgpu_channelizer *c, const cpx *x, cpx *y, int64_t ldy, int64_t F, hipStream_t st);

}  // namespace tsdgpu
