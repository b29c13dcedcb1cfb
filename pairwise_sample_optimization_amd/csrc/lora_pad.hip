// LoRA adapters of rank r < 8: the optimizer's tensors keep peft's shapes (A [r][in], B [out][r], fp32, no pads) while
// the GEMM kernels read working copies zero-padded to the 8-wide rank granule.  Two batched kernels move between the
// two forms, each ONE launch over a device descriptor table that covers every adapter matrix (as pso_transpose_batched):
//   pso_lora_pack:      logical fp32 master -> padded 16-bit working copy (cast, optional B pre-scale, zero pads)
//   pso_lora_grad_fold: padded fp32 gradient scratch -> += into the logical fp32 gradient, scratch cleared
// The logical tensors lie back to back in one flat buffer, so a matrix may start at any 4-byte boundary: 16-byte
// accesses are taken per thread only where the address allows, scalar ones otherwise.  The padded side is always
// 16-byte aligned (Cp % 8 == 0, ld % 8 == 0, 16-byte aligned base: checked where the table is built).
#include "common.h"

struct LoraPadDesc {   // 48 bytes, mirrored by kernels.LoraPadTable
  float* logical;      // [R][C] fp32, rows contiguous (ld = C)
  void* padded;        // [Rp][Cp] with row stride ld: 16-bit elements (pack) or fp32 (fold)
  int R, C, Rp, Cp;
  long ld;
  int scaled;          // pack: 1 for a B matrix (takes the alpha / r pre-scale)
  int reserved;
};

#define GRID_STRIDE_X(i, n) \
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)

// one item = 8 consecutive padded columns of one padded row -> one 16-byte store
__global__ __launch_bounds__(256) void lora_pack_kernel(const LoraPadDesc* __restrict__ d, float scale, int rescale) {
  const LoraPadDesc t = d[blockIdx.y];
  const int cg = t.Cp >> 3;
  const long items = (long)t.Rp * cg;
  bf16_t* dst = reinterpret_cast<bf16_t*>(t.padded);
  GRID_STRIDE_X(i, items) {
    const int r = (int)(i / cg), c0 = (int)(i - (long)r * cg) << 3;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (r < t.R && c0 < t.C) {
      const float* s = t.logical + (long)r * t.C + c0;
      if (c0 + 8 <= t.C && (reinterpret_cast<uintptr_t>(s) & 15) == 0) {
        const float4 a = reinterpret_cast<const float4*>(s)[0], b = reinterpret_cast<const float4*>(s)[1];
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (c0 + j < t.C) v[j] = s[j];
      }
      if (t.scaled && rescale) {
        // the cast, then pso_axpby in the element type (a * x + 0, as that kernel forms it): the same bits as the
        // cast + in-place scale of the unpadded ranks
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = scale * bf_round(v[j]) + 0.f;
      }
    }
    *reinterpret_cast<uint4*>(dst + (long)r * t.ld + c0) =
        make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7]));
  }
}

// one item = 4 consecutive padded columns of one padded row: one 16-byte load, one fp32 add per logical element, one
// 16-byte clear
__global__ __launch_bounds__(256) void lora_grad_fold_kernel(const LoraPadDesc* __restrict__ d) {
  const LoraPadDesc t = d[blockIdx.y];
  const int cg = t.Cp >> 2;
  const long items = (long)t.Rp * cg;
  float* pad = reinterpret_cast<float*>(t.padded);
  GRID_STRIDE_X(i, items) {
    const int r = (int)(i / cg), c0 = (int)(i - (long)r * cg) << 2;
    float4* p = reinterpret_cast<float4*>(pad + (long)r * t.ld + c0);
    if (r < t.R && c0 < t.C) {
      const float4 v = *p;
      float* g = t.logical + (long)r * t.C + c0;
      if (c0 + 4 <= t.C && (reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        float4 a = *reinterpret_cast<float4*>(g);
        a.x += v.x, a.y += v.y, a.z += v.z, a.w += v.w;
        *reinterpret_cast<float4*>(g) = a;
      } else {
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (c0 + j < t.C) g[j] += e[j];
      }
    }
    *p = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

static dim3 lora_pad_grid(int n, long max_items) {
  long bx = (max_items + 255) / 256;
  if (bx > 64) bx = 64;  // grid-stride beyond that: the largest SDXL matrix (8 x 2048) is 8 blocks
  return dim3((unsigned)bx, (unsigned)n, 1);
}

extern "C" {

int pso_lora_pack(int n, const void* descs, long max_items, float scale, void* stream) {
  PSO_ARG_CHECK(n > 0 && n <= 65535 && descs && max_items > 0, "pso_lora_pack: bad args");
  lora_pack_kernel<<<lora_pad_grid(n, max_items), 256, 0, (hipStream_t)stream>>>((const LoraPadDesc*)descs, scale,
                                                                                  scale != 1.0f);
  return pso_check_launch("pso_lora_pack");
}

int pso_lora_grad_fold(int n, const void* descs, long max_items, void* stream) {
  PSO_ARG_CHECK(n > 0 && n <= 65535 && descs && max_items > 0, "pso_lora_grad_fold: bad args");
  lora_grad_fold_kernel<<<lora_pad_grid(n, max_items), 256, 0, (hipStream_t)stream>>>((const LoraPadDesc*)descs);
  return pso_check_launch("pso_lora_grad_fold");
}

}  // extern "C"
