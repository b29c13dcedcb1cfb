// Prodigy optimizer step on the flat fp32 trained buffer (all on device, no host sync).
//
//   Prodigy            prodigyopt 1.0's Prodigy.step for one parameter group -- the optimizer the DreamBooth script
//                      offers as --optimizer prodigy (DB:622-673; its own branch DB:1479-1510 validates the flags and
//                      never constructs the optimizer).  Restated in include/pso_amd.h and tests/prodigy_ref.py; parity
//                      with the package is unpinned (prodigyopt is not available here).
//
// Three launches per step, none of which reads anything back:
//   pass 1     m, v, s with the OLD d, and two fp64 partial sums per workgroup: g (p0 - p) and |s|
//   finalise   one workgroup sums the partials in a fixed order; thread 0 does the scalar algebra in fp64 on the state
//              block (PSO_PRODIGY_*): d_hat, d, d_max, d_numerator, k, the step's dlr and the "updated" flag
//   pass 2     p -= dlr m / (sqrt(v) + d eps) with the NEW d and the old-d dlr, both read from the block
// The per-element arithmetic is fp32 with contraction off, in the order of the restatement; every scalar that enters
// it is formed in fp64 from the block and rounded to fp32 once.  The partial sums are per-thread strided, then wave and
// workgroup trees, then the fixed-order sum of finalise: a step gives the same bits from run to run.
// pso_prodigy_step_lr is the same three launches with lr read from a device word (the learning-rate schedule,
// pso_lr_schedule in optim.hip): pass 1 and finalise load it once per thread in place of the argument.
#include "common.h"

#include <cmath>

#define PRO_THREADS 256
#define PRO_MAX_BLOCKS 2048

#define PRO_D(st, w) (*reinterpret_cast<double*>(reinterpret_cast<int*>(st) + (w)))
#define PRO_CD(st, w) (*reinterpret_cast<const double*>(reinterpret_cast<const int*>(st) + (w)))
#define PRO_I(st, w) (reinterpret_cast<int*>(st)[w])
#define PRO_CI(st, w) (reinterpret_cast<const int*>(st)[w])

struct ProdigyHyper {
  float lr, b1, b2, b3, eps, wd, d_coef, growth;
  int flags;
};

// dlr = d * lr * bc of the step about to be taken (k applied steps so far), fp64; every thread that calls it gets the
// same bits
__device__ __forceinline__ double prodigy_dlr(const void* st, const ProdigyHyper& h) {
#pragma clang fp contract(off)
  double bc = 1.0;
  if (h.flags & PSO_PRODIGY_BIAS_CORRECTION) {
    const double k1 = (double)(PRO_CI(st, PSO_PRODIGY_K) + 1);
    bc = sqrt(1.0 - pow((double)h.b2, k1)) / (1.0 - pow((double)h.b1, k1));
  }
  return PRO_CD(st, PSO_PRODIGY_D) * (double)h.lr * bc;
}

// the factor on the gradient read, and whether the loss scaler skips this step
__device__ __forceinline__ bool prodigy_skip(const float* __restrict__ amp) {
  return amp && reinterpret_cast<const int*>(amp)[PSO_AMP_FOUND_INF] != 0;
}
__device__ __forceinline__ float prodigy_gmul(float gscale, const float* __restrict__ clip,
                                              const float* __restrict__ amp) {
  return amp ? amp[PSO_AMP_GRAD_MUL] * amp[PSO_AMP_CLIP_COEF] : gscale * (clip ? clip[1] : 1.0f);
}

struct ProdigyCoef {
  float gs, cm, cv, cs, b1, b2, b3, wd_g;  // wd_g: the coupled weight decay added to the gradient (0 = none)
};

__device__ __forceinline__ void prodigy_elem1(const ProdigyCoef& c, float graw, float p, float p0, float& m, float& v,
                                              float& s, double& num, double& den) {
#pragma clang fp contract(off)
  float g = graw * c.gs;
  if (c.wd_g != 0.f) g = g + c.wd_g * p;
  num += (double)g * ((double)p0 - (double)p);
  m = c.b1 * m + c.cm * g;
  v = c.b2 * v + (c.cv * g) * g;
  s = c.b3 * s + c.cs * g;
  den += (double)fabsf(s);
}

__global__ __launch_bounds__(PRO_THREADS) void prodigy_pass1_kernel(
    long n, const float* __restrict__ p, const float* __restrict__ g, const float* __restrict__ p0,
    float* __restrict__ m, float* __restrict__ v, float* __restrict__ s, const void* __restrict__ st, ProdigyHyper h,
    float gscale, const float* __restrict__ clip, const float* __restrict__ amp, const float* __restrict__ lr_dev,
    double* __restrict__ part) {
#pragma clang fp contract(off)
  if (prodigy_skip(amp)) return;
  if (lr_dev) h.lr = lr_dev[0];  // pso_prodigy_step_lr: the step's lr from the device word (0 is legal: dlr = 0)
  __shared__ double red[2][PRO_THREADS / 64];
  const double d = PRO_CD(st, PSO_PRODIGY_D), d0 = PRO_CD(st, PSO_PRODIGY_D0);
  const double dlr = prodigy_dlr(st, h);
  ProdigyCoef c;
  c.gs = prodigy_gmul(gscale, clip, amp);
  c.cm = (float)(d * (1.0 - (double)h.b1));
  c.cv = (float)(d * d * (1.0 - (double)h.b2));
  c.cs = (float)((d / d0) * ((h.flags & PSO_PRODIGY_SAFEGUARD_WARMUP) ? d : dlr));
  c.b1 = h.b1;
  c.b2 = h.b2;
  c.b3 = h.b3;
  c.wd_g = (h.flags & PSO_PRODIGY_DECOUPLE) ? 0.f : h.wd;
  double num = 0.0, den = 0.0;
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
  long tail = 0;
  const uintptr_t al = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) |
                       reinterpret_cast<uintptr_t>(p0) | reinterpret_cast<uintptr_t>(m) |
                       reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(s);
  if ((al & 15) == 0) {
    const long n4 = n >> 2;
    for (long i = tid; i < n4; i += nth) {
      const float4 g4 = reinterpret_cast<const float4*>(g)[i];
      const float4 p4 = reinterpret_cast<const float4*>(p)[i];
      const float4 q4 = reinterpret_cast<const float4*>(p0)[i];
      float4 m4 = reinterpret_cast<float4*>(m)[i];
      float4 v4 = reinterpret_cast<float4*>(v)[i];
      float4 s4 = reinterpret_cast<float4*>(s)[i];
      prodigy_elem1(c, g4.x, p4.x, q4.x, m4.x, v4.x, s4.x, num, den);
      prodigy_elem1(c, g4.y, p4.y, q4.y, m4.y, v4.y, s4.y, num, den);
      prodigy_elem1(c, g4.z, p4.z, q4.z, m4.z, v4.z, s4.z, num, den);
      prodigy_elem1(c, g4.w, p4.w, q4.w, m4.w, v4.w, s4.w, num, den);
      reinterpret_cast<float4*>(m)[i] = m4;
      reinterpret_cast<float4*>(v)[i] = v4;
      reinterpret_cast<float4*>(s)[i] = s4;
    }
    tail = n4 << 2;
  }
  for (long i = tail + tid; i < n; i += nth) {
    float mi = m[i], vi = v[i], si = s[i];
    prodigy_elem1(c, g[i], p[i], p0[i], mi, vi, si, num, den);
    m[i] = mi;
    v[i] = vi;
    s[i] = si;
  }
  num = warp_sum_d(num);
  den = warp_sum_d(den);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = num;
    red[1][threadIdx.x >> 6] = den;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0;
    for (int w = 0; w < PRO_THREADS / 64; ++w) {
      a += red[0][w];
      b += red[1][w];
    }
    part[blockIdx.x] = a;
    part[PRO_MAX_BLOCKS + blockIdx.x] = b;
  }
}

// one workgroup: part[0 .. nparts) and part[PRO_MAX_BLOCKS .. + nparts) summed in a fixed order (strided per thread,
// then wave and workgroup trees), then thread 0 updates the state block
__global__ __launch_bounds__(PRO_THREADS) void prodigy_finalise_kernel(int nparts, const double* __restrict__ part,
                                                                       void* __restrict__ st, ProdigyHyper h,
                                                                       const float* __restrict__ amp,
                                                                       const float* __restrict__ lr_dev) {
#pragma clang fp contract(off)
  if (prodigy_skip(amp)) {
    if (threadIdx.x == 0) PRO_I(st, PSO_PRODIGY_SKIPPED) += 1;
    return;
  }
  if (lr_dev) h.lr = lr_dev[0];
  __shared__ double red[2][PRO_THREADS / 64];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
    a += part[i];
    b += part[PRO_MAX_BLOCKS + i];
  }
  a = warp_sum_d(a);
  b = warp_sum_d(b);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = a;
    red[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double dot = 0.0, den = 0.0;
  for (int w = 0; w < PRO_THREADS / 64; ++w) {
    dot += red[0][w];
    den += red[1][w];
  }
  double d = PRO_CD(st, PSO_PRODIGY_D);
  const double d0 = PRO_CD(st, PSO_PRODIGY_D0);
  const double dlr = prodigy_dlr(st, h);
  const double num = (double)h.b3 * PRO_CD(st, PSO_PRODIGY_D_NUMERATOR) + (d / d0) * dlr * dot;
  PRO_D(st, PSO_PRODIGY_DLR) = dlr;
  PRO_D(st, PSO_PRODIGY_D_DENOM) = den;
  if (den == 0.0) {  // nothing to estimate from: the moments stay as pass 1 left them, the parameters are not stepped
    PRO_I(st, PSO_PRODIGY_UPDATED) = 0;
    return;
  }
  const double d_hat = (double)h.d_coef * num / den;
  double d_max = PRO_CD(st, PSO_PRODIGY_D_MAX);
  if (d == d0) d = fmax(d, d_hat);
  d_max = fmax(d_max, d_hat);
  d = fmin(d_max, d * (double)h.growth);
  PRO_D(st, PSO_PRODIGY_D) = d;
  PRO_D(st, PSO_PRODIGY_D_MAX) = d_max;
  PRO_D(st, PSO_PRODIGY_D_NUMERATOR) = num;
  PRO_D(st, PSO_PRODIGY_D_HAT) = d_hat;
  PRO_I(st, PSO_PRODIGY_K) += 1;
  PRO_I(st, PSO_PRODIGY_UPDATED) = 1;
}

__device__ __forceinline__ float prodigy_elem2(float p, float m, float v, float cwd, float dlr, float de) {
#pragma clang fp contract(off)
  if (cwd != 0.f) p = p - cwd * p;
  return p - (dlr * m) / (sqrtf(v) + de);
}

__global__ __launch_bounds__(PRO_THREADS) void prodigy_pass2_kernel(long n, float* __restrict__ p,
                                                                    const float* __restrict__ m,
                                                                    const float* __restrict__ v,
                                                                    const void* __restrict__ st, float eps, float wd,
                                                                    int flags, const float* __restrict__ amp) {
#pragma clang fp contract(off)
  if (prodigy_skip(amp) || !PRO_CI(st, PSO_PRODIGY_UPDATED)) return;
  const double dlr_d = PRO_CD(st, PSO_PRODIGY_DLR);
  const float dlr = (float)dlr_d;
  const float de = (float)(PRO_CD(st, PSO_PRODIGY_D) * (double)eps);
  const float cwd = (flags & PSO_PRODIGY_DECOUPLE) ? (float)((double)wd * dlr_d) : 0.f;
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
  long tail = 0;
  const uintptr_t al =
      reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v);
  if ((al & 15) == 0) {
    const long n4 = n >> 2;
    for (long i = tid; i < n4; i += nth) {
      float4 p4 = reinterpret_cast<float4*>(p)[i];
      const float4 m4 = reinterpret_cast<const float4*>(m)[i];
      const float4 v4 = reinterpret_cast<const float4*>(v)[i];
      p4.x = prodigy_elem2(p4.x, m4.x, v4.x, cwd, dlr, de);
      p4.y = prodigy_elem2(p4.y, m4.y, v4.y, cwd, dlr, de);
      p4.z = prodigy_elem2(p4.z, m4.z, v4.z, cwd, dlr, de);
      p4.w = prodigy_elem2(p4.w, m4.w, v4.w, cwd, dlr, de);
      reinterpret_cast<float4*>(p)[i] = p4;
    }
    tail = n4 << 2;
  }
  for (long i = tail + tid; i < n; i += nth) p[i] = prodigy_elem2(p[i], m[i], v[i], cwd, dlr, de);
}

static int prodigy_blocks(long n) {
  long b = (n + PRO_THREADS - 1) / PRO_THREADS;
  return (int)(b > PRO_MAX_BLOCKS ? PRO_MAX_BLOCKS : (b < 1 ? 1 : b));
}

extern "C" {

size_t pso_prodigy_ws_bytes(long n) { return 2 * PRO_MAX_BLOCKS * sizeof(double); }

// lr_dev != nullptr: the kernels read the step's lr from that device word and `lr` is not used
static int prodigy_launch(const char* who, long n, float* param, const float* grad, const float* p0, float* exp_avg,
                          float* exp_avg_sq, float* s, void* state, float lr, const float* lr_dev, float beta1,
                          float beta2, float beta3, float eps, float weight_decay, int flags, float d_coef,
                          float growth_rate, float grad_scale, const float* clip_coef, const void* amp_state, void* ws,
                          size_t ws_bytes, void* stream) {
  PSO_ARG_CHECK(n > 0 && param && grad && p0 && exp_avg && exp_avg_sq && s && state && ws,
                "%s: bad args (n <= 0 or a null pointer)", who);
  PSO_ARG_CHECK(ws_bytes >= pso_prodigy_ws_bytes(n), "%s: workspace of %zu bytes, need %zu", who, ws_bytes,
                pso_prodigy_ws_bytes(n));
  PSO_ARG_CHECK(((uintptr_t)state & 7) == 0 && ((uintptr_t)ws & 7) == 0 && ((uintptr_t)amp_state & 3) == 0 &&
                    (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)p0 | (uintptr_t)exp_avg |
                      (uintptr_t)exp_avg_sq | (uintptr_t)s | (uintptr_t)clip_coef | (uintptr_t)lr_dev) & 3) == 0,
                "%s: state / ws need 8-B, every other buffer 4-B alignment", who);
  PSO_ARG_CHECK((flags & ~(PSO_PRODIGY_DECOUPLE | PSO_PRODIGY_BIAS_CORRECTION | PSO_PRODIGY_SAFEGUARD_WARMUP)) == 0,
                "%s: unknown flags 0x%x", who, flags);
  const hipStream_t st = (hipStream_t)stream;
  const ProdigyHyper h = {lr, beta1, beta2, beta3, eps, weight_decay, d_coef, growth_rate, flags};
  const float* amp = (const float*)amp_state;
  const int nb = prodigy_blocks(n);
  // weight decay 0 takes neither decay branch (cwd / wd_g == 0)
  prodigy_pass1_kernel<<<nb, PRO_THREADS, 0, st>>>(n, param, grad, p0, exp_avg, exp_avg_sq, s, state, h, grad_scale,
                                                  clip_coef, amp, lr_dev, (double*)ws);
  prodigy_finalise_kernel<<<1, PRO_THREADS, 0, st>>>(nb, (const double*)ws, state, h, amp, lr_dev);
  prodigy_pass2_kernel<<<nb, PRO_THREADS, 0, st>>>(n, param, exp_avg, exp_avg_sq, state, eps, weight_decay, flags,
                                                  amp);
  return pso_check_launch(who);
}

int pso_prodigy_step(long n, float* param, const float* grad, const float* p0, float* exp_avg, float* exp_avg_sq,
                     float* s, void* state, float lr, float beta1, float beta2, float beta3, float eps,
                     float weight_decay, int flags, float d_coef, float growth_rate, float grad_scale,
                     const float* clip_coef, const void* amp_state, void* ws, size_t ws_bytes, void* stream) {
  PSO_ARG_CHECK(lr > 0.0f, "pso_prodigy_step: lr must be positive, got %g", (double)lr);
  return prodigy_launch("pso_prodigy_step", n, param, grad, p0, exp_avg, exp_avg_sq, s, state, lr, nullptr, beta1,
                        beta2, beta3, eps, weight_decay, flags, d_coef, growth_rate, grad_scale, clip_coef, amp_state,
                        ws, ws_bytes, stream);
}

int pso_prodigy_step_lr(long n, float* param, const float* grad, const float* p0, float* exp_avg, float* exp_avg_sq,
                        float* s, void* state, const float* lr_dev, float beta1, float beta2, float beta3, float eps,
                        float weight_decay, int flags, float d_coef, float growth_rate, float grad_scale,
                        const float* clip_coef, const void* amp_state, void* ws, size_t ws_bytes, void* stream) {
  PSO_ARG_CHECK(lr_dev, "pso_prodigy_step_lr: no lr_dev");
  return prodigy_launch("pso_prodigy_step_lr", n, param, grad, p0, exp_avg, exp_avg_sq, s, state, 0.0f, lr_dev, beta1,
                        beta2, beta3, eps, weight_decay, flags, d_coef, growth_rate, grad_scale, clip_coef, amp_state,
                        ws, ws_bytes, stream);
}

}  // extern "C"
