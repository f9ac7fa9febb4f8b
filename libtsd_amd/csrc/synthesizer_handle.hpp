// synthesizer_handle.hpp -- the synthesizer's handle, shared by its four kernel families: the maximally decimated bank
// (synthesizer.hip), the oversampled one (synthesizer_os.hip), the real-output one (synthesizer_real.hip) and the oversampled
// real-output one (synthesizer_real_os.hip).
#pragma once
#include "polybank_host.hpp"

// OS = 1: d_tab f[j][s] = f[j M + s], P = ceil(K / M) rows.  OS > 1: d_tab g[j][r] = f[j D + (r mod D)], P = Q = ceil(K / D) rows.
// HW = (P - 1) M history samples as an (M, P - 1) block: row c channel c's last P - 1 inputs, oldest first
struct tsdgpu_synthesizer : tsdgpu::PolyBank {
  int OS = 1, D = 0;                    // oversampling and hop D = M / OS: a step of F frames makes F D samples
  int phase = 0;                        // hops consumed so far, modulo OS (host side; a launch argument)
  bool real = false;                    // M / 2 + 1 rows into a float32 stream; the history is an (M / 2 + 1, P - 1) block
};

namespace tsdgpu {

// synthesizer_os.hip: one launch of the oversampled kernel (c->OS in {2, 4}) over F frames of hop c->D; reads c->phase
int syn_os_launch(tsdgpu_synthesizer *c, const cpx *u, int64_t ldu, cpx *x, int64_t F, hipStream_t st);

// synthesizer_real.hip: one launch of the real-output kernel (c->real) over F frames of M / 2 + 1 rows into F M floats
int syn_real_launch(tsdgpu_synthesizer *c, const cpx *u, int64_t ldu, float *x, int64_t F, hipStream_t st);

// synthesizer_real_os.hip: one launch of the oversampled real-output kernel (c->real, c->OS in {2, 4}) over F frames of
// M / 2 + 1 rows into F D floats; reads c->phase
int syn_real_os_launch(tsdgpu_synthesizer *c, const cpx *u, int64_t ldu, float *x, int64_t F, hipStream_t st);

// rows a step reads
inline int syn_rows(const tsdgpu_synthesizer *c) { return c->real ? c->M / 2 + 1 : c->M; }

}  // namespace tsdgpu
