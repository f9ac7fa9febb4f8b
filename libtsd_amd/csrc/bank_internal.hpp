// bank_internal.hpp -- what the channel banks share on the host side (bank.hip, rate_bank.hip): the grid's channel limit,
// the overlap test, and the staging of a bank's (C, n) input / output through packed device rows.
#pragma once
#include "common.hpp"

namespace tsdgpu {

struct __attribute__((aligned(4))) f4u { float x, y, z, w; };     // 16 B that global memory may hold at any 4-B boundary

inline int grid_y_limit(int *out)
{
  int dev = 0;
  TSD_HIP(hipGetDevice(&dev));
  TSD_HIP(hipDeviceGetAttribute(out, hipDeviceAttributeMaxGridDimY, dev));
  if (*out <= 0) return set_err(TSDGPU_ERR_HIP, "bank: the device reports a grid y limit of %d", *out);
  return TSDGPU_OK;
}

// [a, a + na) and [b, b + nb) (bytes) share an address
inline bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
  const uintptr_t pa = (uintptr_t) a, pb = (uintptr_t) b;
  return pa < pb + nb && pb < pa + na;
}

// The bank's input / output as device buffers: host data is staged with 2-D copies into packed rows of `ld_s` samples,
// and so are device rows the kernels cannot take as they are (`repack`: in place, or misaligned for the SOS kernel).
inline int bank_stage_in(const void *x, int64_t ldx, int64_t n, int64_t C, size_t sz, bool repack, int64_t ld_s, DevBuf &buf,
                  hipStream_t st, const void **dx, int64_t *dldx)
{
  const bool dev = is_device_ptr(x);
  if (dev && !repack) {
    *dx = x;
    *dldx = ldx;
    return TSDGPU_OK;
  }
  int rc = buf.reserve((size_t) C * (size_t) ld_s * sz);
  if (rc) return rc;
  TSD_HIP(hipMemcpy2DAsync(buf.p, (size_t) ld_s * sz, x, (size_t) ldx * sz, (size_t) n * sz, (size_t) C,
                           dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  *dx = buf.p;
  *dldx = ld_s;
  return TSDGPU_OK;
}
inline int bank_stage_out(void *y, int64_t ldy, int64_t C, size_t sz, bool repack, int64_t ld_s, DevBuf &buf, void **dy,
                   int64_t *dldy, bool *staged)
{
  *staged = repack || !is_device_ptr(y);
  if (!*staged) {
    *dy = y;
    *dldy = ldy;
    return TSDGPU_OK;
  }
  int rc = buf.reserve((size_t) C * (size_t) ld_s * sz);
  if (rc) return rc;
  *dy = buf.p;
  *dldy = ld_s;
  return TSDGPU_OK;
}
inline int bank_finish_out(void *y, int64_t ldy, int64_t n, int64_t C, size_t sz, const void *dy, int64_t dldy, bool staged,
                    hipStream_t st)
{
  if (!staged) return TSDGPU_OK;
  const bool dev = is_device_ptr(y);
  TSD_HIP(hipMemcpy2DAsync(y, (size_t) ldy * sz, dy, (size_t) dldy * sz, (size_t) n * sz, (size_t) C,
                           dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  if (!dev) TSD_HIP(hipStreamSynchronize(st));
  return TSDGPU_OK;
}

}  // namespace tsdgpu

// the overlap-save path of the FIR bank (ols_bank.hip)
struct tsdgpu_fir;
namespace tsdgpu {
int ols_bank_plan(tsdgpu_fir *proto, bool *served, int *grid);
int ols_bank_overlap(const tsdgpu_fir *proto);               // samples of a block that overlap the one before: whole 64-sample rows
bool ols_bank_preferred(const tsdgpu_fir *proto, int64_t n);  // the AUTO rule of a step of n samples per channel
int ols_bank_launch(const tsdgpu_fir *proto, int grid, int64_t C, const void *x, int64_t ldx, void *y, int64_t ldy, int64_t n,
                    const void *hist_old, void *hist_new, int HL, hipStream_t st);
}  // namespace tsdgpu
