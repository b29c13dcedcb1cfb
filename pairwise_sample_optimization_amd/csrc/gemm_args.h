// Kernel argument structs of the GEMM family, shared by gemm.hip (2-phase tiles, dispatch) and gemm8p.hip (8-phase).
#ifndef PSO_GEMM_ARGS_H
#define PSO_GEMM_ARGS_H

#include "common.h"

struct ConvGeom {
  int mode;      // 0 = dense A, else PSO_CONV_* gather
  const bf16_t* src2;  // second channel source (concat) or null
  int C1, C2;    // channels of src1 (A1) and src2
  int H, W;      // input spatial size (source grid)
  int Ho, Wo;    // output spatial size
  int ks, stride, pad;
};

struct GemmArgs {
  const bf16_t* a1; long lda1; int K1;
  const bf16_t* b1; long ldb1;
  const bf16_t* a2; long lda2; int K2;
  const bf16_t* b2; long ldb2;
  int tail_group_n;  // >0: the A2 tail of output columns [j*G, (j+1)*G) starts at A2 column j*K2
  int tail_m;        // rows >= tail_m get no A2 tail (policy + reference images in one pass: LoRA on the first rows)
  int M, N;
  ConvGeom conv;
  float alpha;
  const bf16_t* bias;
  const bf16_t* rowbias; long ld_rowbias; int rows_per_group;
  const bf16_t* resid; long ldr;
  void* out; long ldo; int out_dtype; int accumulate;
  int vec_ok;  // 4-wide epilogue vectors are aligned
  int stage_epi;  // bf16 EPI_NONE epilogue staged through LDS: 16-B coalesced residual loads / output stores
  int group_m;  // tile rows per raster group (>= 1)
  // GEGLU epilogues (diffusers GEGLU: [h | gate] = x W^T + b, out = h * gelu(gate)), weight rows interleaved per 64
  // columns as [h 32 | gate 32]:  EPI_GEGLU writes out = h*gelu(gate) (N/2 columns) and, if out2, the interleaved
  // pre-activation;  EPI_GEGLU_BWD takes the GEMM result as dout (N columns), aux = interleaved pre-activation, and
  // writes the interleaved input gradient [dout*gelu(g) | dout*h*gelu'(g)] to out (2N columns).
  void* out2; long ldo2;
  const bf16_t* aux; long ldaux;
  // batched form (gridDim.z = batch, dense A only): operand z starts batch strides further on (elements)
  long bat_a, bat_b, bat_o;
  int batch;
  // deterministic split-K (gridDim.y > 1 with ws): every split STORES its raw partial acc into ws[split][M][N]
  // (fp32, row pitch N); gemm_splitk_reduce_kernel adds the splits in order and applies the epilogue
  float* ws;
};

struct Gemm8Args {
  const bf16_t* a; long lda;
  const bf16_t* w; long ldw;
  int M, N, K;
  const bf16_t* a2; long lda2; int K2;  // LoRA K-tail (a2 null: none); a2 has tail_m rows
  const bf16_t* w2; long ldw2;
  int tail_m, tail_group_n;              // tail_group_n > 0: column group j takes a2 columns [j*K2, (j+1)*K2)
  float alpha;
  const bf16_t* bias;
  const bf16_t* resid; long ldr;
  void* out; long ldo;
  void* out2; long ldo2; int pre_rows;  // EPI_GEGLU: interleaved pre-activation of rows < pre_rows (optional)
  const bf16_t* aux; long ldaux;        // EPI_GEGLU_BWD: interleaved pre-activation [M][2N]
  int group_m;
  int skip_epi;  // benchmark knob: accumulators kept live, nothing stored (main-loop time alone)
  // FP8 form: E8M0 scale bytes of the rows of A (M), of W (N), of A2 (tail_m) and of W2 (N)
  const uint8_t* sa; const uint8_t* sw; const uint8_t* sa2; const uint8_t* sw2;
  // CONV form (3x3, stride 1, pad 1, NHWC, A = the [B*H*W][C] image with lda = C): image height / width, K-tiles per
  // tap (C / 64) and its 2^20-scaled reciprocal; per-image row bias rowbias[m / (H*W)][N] (the time embedding)
  int cv_H, cv_W, cv_lh, cv_lw, cv_ct, cv_recip;  // H, W powers of two (lh / lw their logs), W >= 8
  const bf16_t* rowbias; long ld_rowbias;
};

// The 8-phase kernels' view of a GEMM / 3x3 convolution described by GemmArgs (the GEGLU pre-activation rows are the
// tail rows: out2 rows < tail_m).  The conv-specific fields beyond H / W are derived by pso_gemm8p_launch.
inline Gemm8Args gemm8_args(const GemmArgs& g) {
  Gemm8Args r{};
  r.a = g.a1; r.lda = g.conv.mode ? g.conv.C1 : g.lda1; r.w = g.b1; r.ldw = g.ldb1;
  r.M = g.M; r.N = g.N; r.K = g.K1;
  r.a2 = g.a2; r.lda2 = g.lda2; r.K2 = g.a2 ? g.K2 : 0; r.w2 = g.b2; r.ldw2 = g.ldb2;
  r.tail_m = g.tail_m; r.tail_group_n = g.a2 ? g.tail_group_n : 0;
  r.alpha = g.alpha; r.bias = g.bias; r.resid = g.resid; r.ldr = g.ldr;
  r.out = g.out; r.ldo = g.ldo; r.out2 = g.out2; r.ldo2 = g.ldo2; r.pre_rows = g.tail_m;
  r.aux = g.aux; r.ldaux = g.ldaux;
  r.group_m = g.group_m;
  r.cv_H = g.conv.H; r.cv_W = g.conv.W;
  r.rowbias = g.rowbias; r.ld_rowbias = g.ld_rowbias;
  return r;
}

// The one host entry of gemm8p.hip for gemm.hip: bn = 256 / 160 / 320 (tile width), epi = EPI8_*, conv = the 3x3
// implicit-GEMM form (bn = 320, plain epilogue).  Preconditions are gemm_plan.h's (N % bn == 0, K % 64 == 0, 16-B
// aligned rows, every operand's M * ld (or N * ld) below 2^30 elements: byte offsets of the buffer loads are 32-bit).
int pso_gemm8p_launch(int bn, int epi, bool conv, Gemm8Args g, hipStream_t st);

#endif  // PSO_GEMM_ARGS_H
