// Merged-weight LoRA / DoRA inference (diffusers fuse_lora, peft merge_and_unload): the adapter folded into a copy of
// the base weight, so a forward on the copy launches nothing for the adapter:
//   O[j][i] = round16( g_j . ( W[j][i] + s . sum_k B[j][k] A[k][i] ) )       (g absent for plain LoRA: no product)
// pso_lora_merge: ONE launch over a device descriptor table, one record per peft module.  It is the element
// pso_dora_weight_norm squares and throws away (dora.hip), stored: fp32 arithmetic on the 16-bit base weight and the
// fp32 MASTERS in peft's shapes (every rank is read as it is), k ascending, one rounding to the element type at the
// end.  No atomics, no LDS, every element is written by exactly one lane: two runs give the same bits.  W is only
// read, so dropping the merged copy is an exact "unfuse".
#include "common.h"

struct LoraMergeDesc {  // 72 bytes, mirrored by kernels.LoraMergeTable
  const bf16_t* W;      // [out][in] 16-bit base weight rows, row stride ldw (8-B aligned rows)
  const float* A;       // [r][in] fp32 master, rows contiguous (16-B aligned)
  const float* B;       // [out][r] fp32 master, rows contiguous (any 4-B boundary)
  const float* g;       // [out] DoRA column scale m / n, or null (plain LoRA)
  bf16_t* O;            // [out][in] 16-bit merged rows, row stride ldo (8-B aligned rows)
  long ldw, ldo;
  int out, in, r;
  float s;              // alpha / r (times lora_scale)
};

#define LORA_MERGE_ROWS 4                            // rows per wave: A's columns are loaded once for all of them
#define LORA_MERGE_BLOCK_ROWS (4 * LORA_MERGE_ROWS)  // 4 waves per block

// One wave owns LORA_MERGE_ROWS rows.  A lane takes 4 consecutive columns at a time (one 8-B load of W, one 16-B load
// of each A row, one 8-B store of O), columns lane * 4 + 256 * t in ascending t.  blockIdx.y is the record, rows are
// grid-strided.  A zero adapter term leaves W's bits alone (W + 0 would turn a -0 into +0).
__global__ __launch_bounds__(256) void lora_merge_kernel(const LoraMergeDesc* __restrict__ d) {
  const LoraMergeDesc t = d[blockIdx.y];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int row0 = (blockIdx.x * 4 + wave) * LORA_MERGE_ROWS; row0 < t.out; row0 += gridDim.x * LORA_MERGE_BLOCK_ROWS) {
    float gs[LORA_MERGE_ROWS];
#pragma unroll
    for (int i = 0; i < LORA_MERGE_ROWS; ++i) {
      const int row = row0 + i < t.out ? row0 + i : t.out - 1;  // clamped: the surplus rows are not stored
      gs[i] = t.g ? t.g[row] : 1.f;
    }
    for (int c = lane * 4; c < t.in; c += 256) {
      float v[LORA_MERGE_ROWS][4];
#pragma unroll
      for (int i = 0; i < LORA_MERGE_ROWS; ++i) v[i][0] = v[i][1] = v[i][2] = v[i][3] = 0.f;
      for (int k = 0; k < t.r; ++k) {
        const float4 a = *reinterpret_cast<const float4*>(t.A + (long)k * t.in + c);
#pragma unroll
        for (int i = 0; i < LORA_MERGE_ROWS; ++i) {
          const int row = row0 + i < t.out ? row0 + i : t.out - 1;
          const float b = t.B[(long)row * t.r + k];
          v[i][0] += b * a.x, v[i][1] += b * a.y, v[i][2] += b * a.z, v[i][3] += b * a.w;
        }
      }
#pragma unroll
      for (int i = 0; i < LORA_MERGE_ROWS; ++i) {
        const int row = row0 + i;
        if (row >= t.out) break;
        const uint2 w = *reinterpret_cast<const uint2*>(t.W + (long)row * t.ldw + c);
        const float w4[4] = {bf2f((bf16_t)(w.x & 0xffff)), bf2f((bf16_t)(w.x >> 16)), bf2f((bf16_t)(w.y & 0xffff)),
                             bf2f((bf16_t)(w.y >> 16))};
        float e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float p = t.s * v[i][j];
          e[j] = p == 0.f ? w4[j] : w4[j] + p;
          if (t.g) e[j] *= gs[i];
        }
        *reinterpret_cast<uint2*>(t.O + (long)row * t.ldo + c) = make_uint2(pack2bf(e[0], e[1]), pack2bf(e[2], e[3]));
      }
    }
  }
}

static bool lora_merge_al(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

extern "C" {

int pso_lora_merge(int n, const void* descs, const void* host_descs, void* stream) {
  PSO_ARG_CHECK(n > 0 && n <= 65535 && descs && host_descs,
                "pso_lora_merge: bad args (n=%d: 1..65535 records, a device table and its host copy)", n);
  const LoraMergeDesc* h = (const LoraMergeDesc*)host_descs;
  int max_out = 0;
  for (int i = 0; i < n; ++i) {
    const LoraMergeDesc& t = h[i];
    PSO_ARG_CHECK(t.out > 0 && t.in > 0 && t.r > 0 && t.W && t.A && t.B && t.O,
                  "pso_lora_merge: record %d: bad args (out=%d in=%d r=%d, W / A / B / O must not be null)", i, t.out,
                  t.in, t.r);
    PSO_ARG_CHECK(t.in % 4 == 0 && lora_merge_al(t.W, 8) && lora_merge_al(t.O, 8) && t.ldw % 4 == 0 &&
                      t.ldo % 4 == 0 && t.ldw >= t.in && t.ldo >= t.in,
                  "pso_lora_merge: record %d: W and O need 8-B aligned rows (in %% 4 == 0, ld %% 4 == 0, ld >= in)", i);
    PSO_ARG_CHECK(lora_merge_al(t.A, 16) && lora_merge_al(t.B, 4) && lora_merge_al(t.g, 4),
                  "pso_lora_merge: record %d: A needs a 16-B boundary, B and g a 4-B one", i);
    if (t.out > max_out) max_out = t.out;
  }
  int bx = cdiv(max_out, LORA_MERGE_BLOCK_ROWS);
  if (bx > 128) bx = 128;  // grid-stride beyond that
  lora_merge_kernel<<<dim3((unsigned)bx, (unsigned)n, 1), 256, 0, (hipStream_t)stream>>>((const LoraMergeDesc*)descs);
  return pso_check_launch("pso_lora_merge");
}

}  // extern "C"
