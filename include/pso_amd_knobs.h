/* Benchmark knobs of the TOOLS build (libpso_amd_knobs.so: the same sources compiled with -DPSO_BENCH_KNOBS).
 *
 * The product library libpso_amd.so (include/pso_amd.h) has none of these: its dispatch is the automatic one, its knob
 * state is compile-time constant, and the measured-not-kept kernel forms are not compiled into it.  The knobs build
 * adds mutable process-wide dispatch overrides for A/B measurements (the tools/ scripts) and for the tests that pin an
 * alternative kernel form to the default's bits (run in a child process: tests/test_knobs_build.py).  Not
 * thread-safe; never on a product path.
 */
#ifndef PSO_AMD_KNOBS_H
#define PSO_AMD_KNOBS_H

#include "pso_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The GEMM variants (csrc/gemm_plan.h decides with them).  The numbers are what the tools and tests pass and never
 * change.  A variant in [PSO_GV_FLIP_FIRST, PSO_GV_FLIP_LAST] keeps the automatic dispatch and flips one of its rules;
 * every other non-zero one turns the automatic 8-phase and skinny rules off, and 1-29 also force one 2-phase tile
 * BM x BN, WM x WN waves, STAGES-deep ring (p = the register-pipelined schedule). */
enum PsoGemmVariant {
  PSO_GV_AUTO = 0,
  PSO_GV_T256x128_4x2_S3 = 1,
  PSO_GV_T128x128_2x2_S3 = 2,
  PSO_GV_T128x128_2x2 = 3,
  PSO_GV_T256x256 = 4,
  PSO_GV_T256x128 = 5,
  PSO_GV_T64x128 = 6,
  PSO_GV_T128x256 = 7,
  PSO_GV_T128x128 = 8,
  PSO_GV_T256x256_P = 10,
  PSO_GV_T128x128_P = 11,
  PSO_GV_T128x160 = 12,
  PSO_GV_T256x160 = 14,
  PSO_GV_T256x160_P = 16,
  PSO_GV_T128x320 = 17,
  PSO_GV_T256x320 = 18,
  PSO_GV_T128x160_P = 19,
  PSO_GV_T64x160 = 20,
  PSO_GV_T128x80_4x1 = 21,
  PSO_GV_T64x160_S3 = 22,
  PSO_GV_T64x160_S4 = 23,
  PSO_GV_T64x160_S5 = 24,
  PSO_GV_T64x64_S4 = 25,
  PSO_GV_T128x160_S4 = 26,
  PSO_GV_T64x128_S4 = 27,
  PSO_GV_T128x128_S4 = 28,
  PSO_GV_T64x64_S5 = 29,
  PSO_GV_FORCE_8P256 = 30,        /* the 8-phase 256 x 256 form wherever it applies */
  PSO_GV_NO_8P = 31,              /* no 8-phase form anywhere (GEMM, GEGLU forward and backward) */
  PSO_GV_8P256_ANY_N = 32,        /* the 8-phase 256 x 256 form from one round of tiles at any N % 256 == 0 */
  PSO_GV_GEGLU_T128x128 = 33,     /* 33-36: 2-phase tiles of the GEGLU forward (8-phase off) */
  PSO_GV_GEGLU_T128x256 = 34,
  PSO_GV_GEGLU_T256x128_4x2 = 35,
  PSO_GV_GEGLU_T128x128_S3 = 36,
  PSO_GV_FLIP_FIRST = 37,
  PSO_GV_8P160_OFF = 37,          /* keep the 2-phase 128 x 160 where the 8-phase 256 x 160 is the default */
  PSO_GV_FORCE_8P160 = 38,        /* the 8-phase 256 x 160 form wherever it applies */
  PSO_GV_FORCE_8P320 = 39,        /* the 8-phase 256 x 320 form wherever it applies */
  PSO_GV_8P320_OFF = 40,          /* the 8-phase 256 x 320 form off */
  PSO_GV_LANE_EPILOGUE = 41,      /* the per-lane 8-B epilogue instead of the LDS-staged 16-B one */
  PSO_GV_8P320_SHORT_K = 42,      /* the 8-phase 256 x 320 form only for K < 2560 */
  PSO_GV_CONV8_OFF = 43,          /* 3x3 convolutions stay on the 2-phase kernel */
  PSO_GV_FORCE_CONV8 = 44,        /* 3x3 convolutions on the 8-phase 256 x 320 tiles wherever they apply */
  PSO_GV_GEGLU_BWD_320_OFF = 45,  /* the GEGLU backward keeps the 256 x 256 form */
  PSO_GV_ROUND2_RULES = 46,       /* no wide-N 320 form, full-round 320 rules, no 128 x 128 for 384-511 tiles */
  PSO_GV_8P320_FULL_ROUND = 47,   /* the 8-phase 256 x 320 forms (GEMM and conv) only from a full round of tiles */
  PSO_GV_KEEP_T128x160 = 48,      /* no 64 x 160 tiles where 128 x 160 make at most one workgroup per CU */
  PSO_GV_SMALL_M_T128x128_P = 49, /* the pipelined 128 x 128 tiles for the small-M short-K products */
  PSO_GV_8P256_FULL_ROUND = 50,   /* no 8-phase 256 x 256 at three quarters of a round */
  PSO_GV_SPLIT_MIN_8 = 51,        /* workspace split-K from 8 K-tiles per split */
  PSO_GV_CONV_SPLIT_OFF = 52,     /* the workspace split-K forms off (pso_gemm_ws / pso_conv2d_ws) */
  PSO_GV_SPLIT_HALF_ROUND = 55,   /* workspace split-K only up to half a round of tiles */
  PSO_GV_TN256_OFF = 56,          /* the TN products keep the 128 x 128 tiles */
  PSO_GV_GEGLU_KEEP_256 = 57,     /* the GEGLU forward keeps the 256 x 256 form */
  PSO_GV_GEGLU_320_EQUAL = 58,    /* the GEGLU forward takes 256 x 320 at equal rounds too */
  PSO_GV_FLIP_LAST = 58
};

/* GEMM dispatch override: v % 100 = variant (enum PsoGemmVariant; 0 = automatic per shape), v / 100 = raster-group
 * rows (0 = automatic). */
void pso_gemm_set_variant(int v);
/* What csrc/gemm_plan.h decides for a problem, without launching or touching a device.  The problem is given by
 * value: shapes, row pitches and the byte alignment of each pointer (0 = operand absent); the knobs are arguments,
 * not the process's knob state.  kind selects the entry whose decision is asked for. */
enum PsoGemmPlanKind {
  PSO_PLAN_GEMM = 0,      /* pso_gemm; pso_gemm_ws with have_ws */
  PSO_PLAN_CONV = 1,      /* pso_conv2d; pso_conv2d_ws with have_ws */
  PSO_PLAN_BATCHED = 2,   /* pso_gemm_batched */
  PSO_PLAN_GEGLU = 3,     /* pso_gemm_geglu (N = 2 F interleaved columns) */
  PSO_PLAN_GEGLU_BWD = 4, /* pso_gemm_geglu_bwd */
  PSO_PLAN_TN = 5,        /* pso_gemm_tn / _grouped (group) / _ws (have_ws); M = reduction rows, N = I, K1 = J */
  PSO_PLAN_TN_GEGLU = 6   /* pso_gemm_tn_geglu; M = reduction rows, N = F2, K1 = J */
};
typedef struct {
  int variant, group, tn_split; /* the knobs */
  int have_ws;                  /* a 16-B aligned workspace large enough for the plan's splits was supplied */
  int M, N, K1, K2;             /* K2 > 0: a second operand pair (LoRA K-tail) */
  long lda1, ldb1, lda2, ldb2;
  int tail_group_n, tail_rows, batch, out_dtype, accumulate;
  int bias_align, rowbias_align, resid_align, out_align; /* bytes; 0 = absent */
  long ld_rowbias, ldr, ldo;
  int rows_per_group;
  float alpha;
  int conv_mode, B, C1, C2, H, W, Ho, Wo, ks, stride, pad; /* PSO_PLAN_CONV (M, N = Cout, K1 are derived) */
  int tn_group;                                            /* PSO_PLAN_TN: pso_gemm_tn_grouped's group */
} PsoGemmPlanQuery;
typedef struct {
  int form;     /* gemm_plan.h GemmForm; PSO_PLAN_TN: TnKind */
  int bm, bn, wm, wn, stages, pipe; /* 2-phase tile (form GF_TILE); bn also the 8-phase tile width */
  int epi;      /* 0 plain, 1 GEGLU, 2 GEGLU backward */
  int conv_mode;
  int atomic_ks, ws_ks; /* split-K counts: f32 atomics / ordered through the workspace (0, 1: none) */
  int stage_epi, vec_ok, group_m;
} PsoGemmPlanInfo;
int pso_gemm_plan_query(int kind, const PsoGemmPlanQuery* q, PsoGemmPlanInfo* info);
/* 8-phase kernels: bit 0 = keep the accumulators live but store nothing (main-loop cost), bits 1-2 = wave-group
 * schedule (lockstep / static priority). */
void pso_gemm8p_skip_epilogue(int on);
/* Split count of pso_gemm_tn over the reduction rows (0 = automatic). */
void pso_gemm_tn_set_split(int ks);
/* Attention: ones digit = forward form (0 auto, 1 lane-local growth test, 2 / 4 force 32 / 64 rows per wave, 5-9 the
 * first-round loop), tens digit = backward form (0 default, 1 / 3 older forms, 4 64 keys per wave, 5 / 6 deeper
 * rings, 7 the dQ + dK/dV launches for short key sequences too (instead of the one-pass attn_bwd_x_kernel), 8 / 9 the
 * 8-wave ping-pong dK/dV), 100s = VALU row sums, 1000s = segment clock trace of the ping-pong form, 10000 * qs = the
 * query splits of attn_bwd_x_kernel (0 automatic). */
void pso_attention_set_variant(int v);
/* Segment-start clocks of the last traced ping-pong dK/dV launch (2 x 520 unsigned 64-bit, group-major). */
int pso_attn_pp_trace(unsigned long long* out);

#ifdef __cplusplus
}
#endif

#endif /* PSO_AMD_KNOBS_H */
