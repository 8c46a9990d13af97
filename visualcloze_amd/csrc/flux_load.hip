// vc_flux_load_finish's last launch: every QK-norm scale vector of a checkpoint (RMSNorm.scale, modules/layers.py:63-73: 128 values,
// bf16 or f32 as stored) cast to bf16 where vc_flux_bind_weight wants it, and max|.| of the CAST values, one f32 per vector - what
// `p.to(bfloat16)` and `t.float().abs().max()` give (a NaN anywhere makes the maximum NaN, as torch's max does).  One workgroup of
// 128 threads per vector; up to VC_SCALE_VECTORS vectors per launch travel as kernel arguments (FLUX.1: 152), so nothing is staged.
#include "common.h"
#include "vcloze_internal.h"

namespace {

__global__ __launch_bounds__(128) void scale_cast_kernel(const VcScaleVectors v, bf16_t* out, int64_t out_stride, float* amax) {
  __shared__ float part[2];
  __shared__ int bad[2];
  const int i = blockIdx.x, t = threadIdx.x;
  const float x = v.f32[i] ? ((const float*)v.src[i])[t] : bf2f(((const bf16_t*)v.src[i])[t]);
  const bf16_t b = x != x ? (bf16_t)0x7fc0 : f2bf(x);       // torch's cast makes every NaN this one
  out[i * out_stride + t] = b;
  const float a = fabsf(bf2f(b));
  const bool nan = a != a;
  float m = nan ? 0.0f : a;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  const int any = __any(nan);
  if ((t & 63) == 0) { part[t >> 6] = m; bad[t >> 6] = any; }
  __syncthreads();
  if (t == 0) amax[i] = bad[0] || bad[1] ? __builtin_nanf("") : fmaxf(part[0], part[1]);
}

}  // namespace

int vc_scale_cast_launch(const VcScaleVectors& v, int n, void* out, int64_t out_stride, float* amax, hipStream_t s, char* err, int errlen) {
  if (n <= 0 || n > VC_SCALE_VECTORS || !out || !amax || out_stride < 128) {
    snprintf(err, errlen, "scale_cast: bad arguments (n = %d)", n);
    return VC_ERR_ARG;
  }
  for (int i = 0; i < n; ++i)
    if (!v.src[i]) { snprintf(err, errlen, "scale_cast: null vector %d", i); return VC_ERR_ARG; }
  hipLaunchKernelGGL(scale_cast_kernel, dim3(n), dim3(128), 0, s, v, (bf16_t*)out, out_stride, amax);
  return vc_launch_status("scale_cast", err, errlen);
}
