// channelizer_internal.hpp -- the shapes the polyphase banks serve and the geometry of their LDS image.
#pragma once
#include <cstddef>

namespace tsdgpu {

constexpr int CHAN_MIN_M = 8, CHAN_MAX_M = 1024;   // channels: a power of two in this range
constexpr int CHAN_MAX_P = 16;                     // taps per hop sample: K <= 16 D, D = M / OS the hop (K <= 16 M at OS = 1)
constexpr int CHAN_NT = 512;                       // threads of a workgroup, analysis and synthesis

// the real banks transform at M / 2, one position per thread: M / 2 in [8, 512]
constexpr int CHAN_REAL_MIN_M = 2 * CHAN_MIN_M;

inline bool chan_served_channels(int M, int min_M) { return M >= min_M && M <= CHAN_MAX_M && (M & (M - 1)) == 0; }

// oversampling OS = M / D of the analysis bank: 1 (maximally decimated), 2, 4
inline bool chan_served_oversample(int OS) { return OS == 1 || OS == 2 || OS == 4; }

// first radix of the transform M = R0 16^a (stockham16.hpp); 0: M = 8, one dft8 per frame
inline int chan_radix0(int M)
{
  if (M == 8) return 0;
  while (M > 16) M >>= 4;
  return M;
}

// Pitch of a frame in the LDS image, in samples.  A frame holds its M points at i + i / 16 (stockham16.hpp).  The read-back
// takes 8 frame pairs x 8 neighbouring channels per wave instruction: the pitch is 4 modulo 16 where the 160 KiB allow it
// (pair k, channel c at bank pair 8 k + c), and odd below M = 32.
inline int chan_frame_pitch(int M)
{
  const int pn = M + (M >> 4);
  if (M < 32) return pn | 1;
  return pn + ((4 - pn) & 15);
}

// a workgroup of NT threads holds 16 frames of each of its NT / M sub-runs
inline size_t chan_lds_bytes(int NT, int M, int FP) { return (size_t) (16 * NT / M) * (size_t) FP * 8; }

}  // namespace tsdgpu
