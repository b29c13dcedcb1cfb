// Exponential moving average of the flat fp32 trained buffer (all on device, no host sync).
//
//   EMA step    diffusers' EMAModel.step for one tensor: s_param.sub_(one_minus_decay * (s_param - param)).  The decay is
//               evaluated on the host in double (ema.py get_decay) and travels as one float; restated in
//               include/pso_amd.h and tests/ema_ref.py.  Parity with the package is unpinned (diffusers is not
//               available here).
//   swap        exchanges two buffers in one pass: store / copy_to / restore without a third copy of the master (10 GB in
//               the full-UNet mode).
// Both are grid-stride loops with 64-bit indices (the full-UNet master has 2.57e9 elements); operands 16-B aligned take
// 16-B loads and stores with a scalar tail, others 4-B ones (the rule of optim.hip and prodigy.hip).  The element
// arithmetic is three separately rounded fp32 operations: no contraction, since a fused s - omd t rounds once where the
// restatement rounds twice.
#include "common.h"

#include <cmath>

#define EMA_THREADS 256
#define EMA_MAX_BLOCKS 2048

__device__ __forceinline__ float ema_elem(float s, float p, float omd) {
  // plain operators under the pragma, as prodigy.hip's: the __fsub_rn / __fmul_rn of the HIP headers are inline
  // functions compiled under the default contraction, and once inlined here the compiler fuses them (checked in the
  // ISA: v_fma_f32 with them, v_mul_f32 + v_sub_f32 without)
#pragma clang fp contract(off)
  const float t = s - p;
  const float u = omd * t;
  return s - u;
}

__global__ __launch_bounds__(EMA_THREADS) void ema_step_kernel(long n, float* __restrict__ s,
                                                               const float* __restrict__ p, float omd) {
#pragma clang fp contract(off)
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
  long tail = 0;
  const uintptr_t al = reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(p);
  if ((al & 15) == 0) {
    const long n4 = n >> 2;
    for (long i = tid; i < n4; i += nth) {
      float4 s4 = reinterpret_cast<float4*>(s)[i];
      const float4 p4 = reinterpret_cast<const float4*>(p)[i];
      s4.x = ema_elem(s4.x, p4.x, omd);
      s4.y = ema_elem(s4.y, p4.y, omd);
      s4.z = ema_elem(s4.z, p4.z, omd);
      s4.w = ema_elem(s4.w, p4.w, omd);
      reinterpret_cast<float4*>(s)[i] = s4;
    }
    tail = n4 << 2;
  }
  for (long i = tail + tid; i < n; i += nth) s[i] = ema_elem(s[i], p[i], omd);
}

// a and b do not overlap (the entry refuses it): every element is read and written by one thread only
__global__ __launch_bounds__(EMA_THREADS) void ema_swap_kernel(long n, float* __restrict__ a, float* __restrict__ b) {
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
  long tail = 0;
  const uintptr_t al = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b);
  if ((al & 15) == 0) {
    const long n4 = n >> 2;
    for (long i = tid; i < n4; i += nth) {
      const float4 a4 = reinterpret_cast<const float4*>(a)[i];
      const float4 b4 = reinterpret_cast<const float4*>(b)[i];
      reinterpret_cast<float4*>(a)[i] = b4;
      reinterpret_cast<float4*>(b)[i] = a4;
    }
    tail = n4 << 2;
  }
  for (long i = tail + tid; i < n; i += nth) {
    const float ai = a[i], bi = b[i];
    a[i] = bi;
    b[i] = ai;
  }
}

// one float4 per thread up to EMA_MAX_BLOCKS workgroups, the grid-stride loop beyond
static int ema_blocks(long n) {
  long b = ((n + 3) / 4 + EMA_THREADS - 1) / EMA_THREADS;
  return (int)(b > EMA_MAX_BLOCKS ? EMA_MAX_BLOCKS : (b < 1 ? 1 : b));
}

extern "C" {

int pso_ema_step(long n, float* shadow, const float* param, float one_minus_decay, void* stream) {
  PSO_ARG_CHECK(n > 0 && shadow && param, "pso_ema_step: bad args (n <= 0 or a null pointer)");
  PSO_ARG_CHECK((((uintptr_t)shadow | (uintptr_t)param) & 3) == 0, "pso_ema_step: buffers need 4-B alignment");
  PSO_ARG_CHECK(std::isfinite(one_minus_decay) && one_minus_decay >= 0.0f && one_minus_decay <= 1.0f,
                "pso_ema_step: one_minus_decay must lie in [0, 1], got %g", (double)one_minus_decay);
  ema_step_kernel<<<ema_blocks(n), EMA_THREADS, 0, (hipStream_t)stream>>>(n, shadow, param, one_minus_decay);
  return pso_check_launch("pso_ema_step");
}

int pso_ema_swap(long n, float* a, float* b, void* stream) {
  PSO_ARG_CHECK(n > 0 && a && b, "pso_ema_swap: bad args (n <= 0 or a null pointer)");
  PSO_ARG_CHECK(a + n <= b || b + n <= a, "pso_ema_swap: a and b are the same buffer or overlap");
  PSO_ARG_CHECK((((uintptr_t)a | (uintptr_t)b) & 3) == 0, "pso_ema_swap: buffers need 4-B alignment");
  ema_swap_kernel<<<ema_blocks(n), EMA_THREADS, 0, (hipStream_t)stream>>>(n, a, b);
  return pso_check_launch("pso_ema_swap");
}

}  // extern "C"
