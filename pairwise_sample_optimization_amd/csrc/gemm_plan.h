// Which GEMM kernel runs: the decision of gemm.hip as plain host C++ (no HIP, no pointers, no process state).
//
//   facts (GemmFacts: shapes, epilogue, alignment classes -- values only)  +  knobs (GemmKnobs)  ->  GemmPlan
//
// gemm.hip fills the facts from its argument struct (gemm_facts, the only place that looks at pointers), asks for the
// plan and launches what it says; the tools build answers the same question without a device (pso_gemm_plan_query,
// include/pso_amd_knobs.h), and tests/test_gemm_plan_cpu.py pins every rule here to a recorded table
// (tests/golden/gemm_dispatch_table.json).  Every threshold below carries the measurement that set it.
#ifndef PSO_GEMM_PLAN_H
#define PSO_GEMM_PLAN_H

#include <cstddef>

#include "../../include/pso_amd_knobs.h"

// Benchmark knobs (A/B variants, forced tiles, raster groups, the TN split): only the tools build (-DPSO_BENCH_KNOBS ->
// libpso_amd_knobs.so, include/pso_amd_knobs.h) has them as mutable state; the product and fp16 libraries pass a
// constexpr all-zero value, so every knob branch folds away and the measured-not-kept forms are not compiled into them.
struct GemmKnobs {
  int variant = 0;   // enum PsoGemmVariant
  int group = 0;     // raster group rows (0 = automatic)
  int tn_split = 0;  // split count of the 64 x 64 TN kernel (0 = automatic); non-zero also keeps the TN products off
                     // the rank-r, 128 x 128 and 256 x 256 kernels
  bool tn128_off = false;  // the 64 x 64 TN kernel instead of the atomic 128 x 128 one (PSO_TN128=0)
};

// a variant that flips one rule of the automatic dispatch (which otherwise stays on), as opposed to one that forces a
// tile shape or form (41 = per-lane epilogue; 37 / 38 = the 256 x 160 8-phase tiles off / forced; 56 = the 256 x 256
// TN tiles off; ...)
constexpr bool gemm_variant_flips_rule(int v) { return v >= PSO_GV_FLIP_FIRST && v <= PSO_GV_FLIP_LAST; }
// 0 where the automatic rules are on, else the forcing variant
constexpr int gemm_forcing_variant(int v) { return gemm_variant_flips_rule(v) ? 0 : v; }
// the workspace split-K forms (pso_gemm_ws / pso_conv2d_ws) under the benchmark knobs: off where a variant forces a
// tile (38 / 39 / 44: the 8-phase 256 x 160 / 256 x 320 / conv tiles, the tests that pin them), where a raster group
// is forced, and under variant 52 (the conv split off)
constexpr bool gemm_ws_allowed(const GemmKnobs& k) {
  return k.group == 0 && gemm_forcing_variant(k.variant) == 0 && k.variant != PSO_GV_FORCE_8P160 &&
         k.variant != PSO_GV_FORCE_8P320 && k.variant != PSO_GV_FORCE_CONV8 && k.variant != PSO_GV_CONV_SPLIT_OFF;
}

// raster group rows: C2-step sweep (tools/_var_ab.sh, same box) 2 / 3 / 4 / 5 / 6 / 8 / 16 -> 240.4 / 239.7 / 239.1 /
// 239.2 / 238.9 / 240.5 / 241.9 ms
#define PSO_GEMM_GROUP_M 4

struct GemmFacts {
  int M, N, K1, K2;  // K2 = 0 without a second operand pair
  bool has_tail;     // second operand pair (LoRA K-tail) present
  int tail_group_n, tail_m, batch, out_dtype, accumulate;
  bool has_bias, has_rowbias, has_resid;
  // conv geometry (mode 0: dense A); B images
  int conv_mode, B, C1, C2, H, W, Ho, Wo, ks, stride, pad;
  // alignment classes; those of an absent operand are true
  bool ab16;      // A1, B1 16-B aligned
  bool ld_ab8;    // lda1 % 8 == 0 && ldb1 % 8 == 0
  bool ld_ab_eq;  // lda1 == ldb1
  bool out16, out_vec;  // out 16-B aligned; aligned for a 4-wide vector of its type (f32: 16 B, 16-bit: 8 B)
  bool ldo8, ldo4;
  bool resid16;   // resid 16-B aligned rows (pointer and ldr % 8 == 0)
  bool resid8;    // resid 8-B aligned rows (pointer and ldr % 4 == 0)
  bool bias8, rowbias8, ld_rowbias4;
  bool rowgroup_hw;  // rows_per_group == Ho * Wo
  // 32-bit byte offsets of the buffer loads: rows * ld < 2^30 elements
  bool fits_a, fits_b;  // M x lda1, N x ldb1
  bool fits_tail;       // tail_m x lda2 and N x ldb2
  bool fits_conv;       // (M + 2 (W + 1)) x C1
  // a 16-B aligned workspace of ws_bytes was supplied (pso_gemm_ws / pso_conv2d_ws)
  bool have_ws;
  size_t ws_bytes;
  // pso_conv2d may take the direct small-Cout convolution: alpha == 1, ldo == Cout (pso_conv2d_ws never does)
  bool small_conv_entry;
};

enum GemmForm {
  GF_NONE = 0,    // nothing to launch (M or N == 0)
  GF_TILE,        // 2-phase gemm_bf16_kernel<BM, BN, conv, WM, WN, STAGES, PIPE, EPI>
  GF_8P256,       // 8-phase 256 x 256 (gemm8p.hip)
  GF_8P160,       // 8-phase 256 x 160
  GF_8P320,       // 8-phase 256 x 320
  GF_8P320_CONV,  // 8-phase 256 x 320, 3x3 implicit-GEMM convolution
  GF_SKINNY,      // N <= 128 without epilogue operands (gemm_skinny.hip picks its own inner form)
  GF_SMALL_CONV,  // Cout <= 3 direct 3x3 convolution (conv_small.hip)
  GF_FORMS
};
enum { GEPI_NONE = 0, GEPI_GEGLU = 1, GEPI_GEGLU_BWD = 2 };

struct GemmPlan {
  int form = GF_NONE;
  int BM = 0, BN = 0, WM = 0, WN = 0, STAGES = 0;  // GF_TILE; BN also the 8-phase tile width
  bool PIPE = false;
  int epi = GEPI_NONE;
  int atomic_ks = 1;  // split-K over gridDim.y with f32 atomics in the epilogue
  int ws_ks = 0;      // >= 2: deterministic split-K through the workspace, reduced in split order
  bool stage_epi = false, vec_ok = false;
  int group_m = PSO_GEMM_GROUP_M;
  constexpr bool tile_is(int bm, int bn, int wm, int wn, int st, bool pipe) const {
    return BM == bm && BN == bn && WM == wm && WN == wn && STAGES == st && PIPE == pipe;
  }
};

constexpr GemmPlan& plan_tile(GemmPlan& p, int bm, int bn, int wm = 2, int wn = 2, int st = 2, bool pipe = false) {
  p.form = GF_TILE; p.BM = bm; p.BN = bn; p.WM = wm; p.WN = wn; p.STAGES = st; p.PIPE = pipe;
  return p;
}
constexpr GemmPlan& plan_8p(GemmPlan& p, int form, int bn) {
  p.form = form; p.BN = bn;
  return p;
}

// Split-K plan of a dense GEMM whose output tiles leave CUs idle while its reduction is long (the bs = 1 / GPU
// backward at M = 2048: 2048 x 1280 x 10240 makes 128 tiles of 128 x 160 -- half a 256-CU round at one workgroup
// each; and one-round shapes with K >= 4096): ks K-splits of >= 16 K-tiles each, towards 512 workgroups (two per
// CU), reduced in split order through a
// caller-owned fp32 workspace (deterministic).  The partials cost 8 M N bytes per split against 2 M N K / ks flop,
// so only K >= 2048 qualifies.  Returns ks (0: no split) and the tile.
struct SplitPlan { int ks, bm, bn; };
constexpr SplitPlan gemm_split_plan(int M, int N, int K1, int K2, bool has_tail, const GemmKnobs& k) {
  SplitPlan p{0, 0, 0};
  if (M <= 0 || N <= 0 || (N % 4) != 0) return p;
  const int bm = 128, bn = (N % 160) == 0 ? 160 : 128;
  const long tiles = (long)((M + bm - 1) / bm) * ((N + bn - 1) / bn);
  const int nt_all = (K1 + 63) / 64 + (has_tail ? (K2 + 63) / 64 : 0);
  // variant 51: splits of >= 8 K-tiles (the short-K M = 2048 products: 2048 x 1280 x 1280 + LoRA in two)
  const int min_kt = k.variant == PSO_GV_SPLIT_MIN_8 ? 8 : 16;
  // one full round of tiles (<= 256: the 4096-row products and 3x3 convs of the bs = 1 / GPU pass, K >= 4096) splits
  // in two as well: bs = 1 step 81.56 -> 80.25 ms, C3 237.2 -> 236.5, C2 untouched (tools/bs1_variant_ab.py, one box;
  // K >= 2560 measured the same, up to 384 tiles cost C3 1.5 %).  Variant 55 keeps the half-round rule.
  const bool round2 = k.variant != PSO_GV_SPLIT_HALF_ROUND && tiles <= 256 && nt_all >= 64;
  if ((tiles > 128 && !round2) || nt_all < 2 * min_kt) return p;
  int ks = (int)((512 + tiles - 1) / tiles);
  if (ks > nt_all / min_kt) ks = nt_all / min_kt;
  if (ks < 2) return p;
  p.ks = ks; p.bm = bm; p.bn = bn;
  return p;
}

// The forced 2-phase tiles (A/B and tests; gemm.hip instantiates them in the tools build only):
// X(variant, the tail-group / width condition it needs, BM, BN, WM, WN, STAGES, PIPE)
#define PSO_FORCED_TILES(X)                                        \
  X(PSO_GV_T256x256, bn256_ok, 256, 256, 2, 4, 2, false)           \
  X(PSO_GV_T256x128, !bn64_only, 256, 128, 2, 4, 2, false)         \
  X(PSO_GV_T256x128_4x2_S3, !bn64_only, 256, 128, 4, 2, 3, false)  \
  X(PSO_GV_T128x128_2x2_S3, !bn64_only, 128, 128, 2, 2, 3, false)  \
  X(PSO_GV_T128x128_2x2, !bn64_only, 128, 128, 2, 2, 2, false)     \
  X(PSO_GV_T64x128, !bn64_only, 64, 128, 2, 2, 2, false)           \
  X(PSO_GV_T128x256, bn256_ok, 128, 256, 2, 4, 2, false)           \
  X(PSO_GV_T128x128, !bn64_only, 128, 128, 2, 4, 2, false)         \
  X(PSO_GV_T256x256_P, bn256_ok, 256, 256, 2, 4, 2, true)          \
  X(PSO_GV_T128x128_P, !bn64_only, 128, 128, 2, 4, 2, true)        \
  X(PSO_GV_T128x160, n160, 128, 160, 2, 2, 2, false)               \
  X(PSO_GV_T256x160, n160, 256, 160, 2, 2, 2, false)               \
  X(PSO_GV_T256x160_P, n160, 256, 160, 2, 2, 2, true)              \
  X(PSO_GV_T128x320, n320, 128, 320, 2, 4, 2, false)               \
  X(PSO_GV_T256x320, n320, 256, 320, 2, 4, 2, false)               \
  X(PSO_GV_T128x160_P, n160, 128, 160, 2, 2, 2, true)              \
  /* small-M tiles (the bs = 1 backward at M = 2048: N = 1280 makes one 256-CU round of 64 x 160 / 128 x 80) */ \
  X(PSO_GV_T64x160, n160, 64, 160, 2, 2, 2, false)                 \
  X(PSO_GV_T128x80_4x1, n80, 128, 80, 4, 1, 2, false)              \
  X(PSO_GV_T64x160_S3, n160, 64, 160, 2, 2, 3, false)              \
  /* deeper direct-to-LDS rings for the latency-bound short-K small-M products (3 / 4 K-tiles in flight) */ \
  X(PSO_GV_T64x160_S4, n160, 64, 160, 2, 2, 4, false)              \
  X(PSO_GV_T64x160_S5, n160, 64, 160, 2, 2, 5, false)              \
  X(PSO_GV_T64x64_S4, !bn64_only, 64, 64, 2, 2, 4, false)          \
  X(PSO_GV_T128x160_S4, n160, 128, 160, 2, 2, 4, false)            \
  X(PSO_GV_T64x128_S4, !bn64_only, 64, 128, 2, 2, 4, false)        \
  X(PSO_GV_T128x128_S4, !bn64_only, 128, 128, 2, 4, 4, false)      \
  X(PSO_GV_T64x64_S5, !bn64_only, 64, 64, 2, 2, 5, false)

constexpr GemmPlan gemm_plan(const GemmFacts& f, const GemmKnobs& k) {
  GemmPlan p;
  const int gv_raw = k.variant;
  const int gv = gemm_forcing_variant(gv_raw);
  const bool conv3x3_same = f.conv_mode == PSO_CONV_NORMAL && f.ks == 3 && f.stride == 1 && f.pad == 1 &&
                            f.H == f.Ho && f.W == f.Wo && f.C2 == 0 && !f.has_tail && f.out_dtype != PSO_F32 &&
                            !f.accumulate;
  // Cout <= 3 (the VAE decoder's conv_out to RGB): a direct convolution instead of an N = 3 GEMM padded to 64-column
  // MFMA tiles (conv_small.hip; 1024^2: 1.34 ms -> see DESIGN §4 / profiles/r06_vae_conv_out_ab.log)
  if (f.small_conv_entry && conv3x3_same && !f.has_rowbias && !f.has_resid && f.N >= 1 && f.N <= 3 &&
      (f.H % 16) == 0 && (f.W % 16) == 0 && (f.C1 % 64) == 0 && f.B >= 1 && f.B <= 65535 &&
      (long)f.B * f.H * f.W * f.C1 < (1L << 31)) {
    p.form = GF_SMALL_CONV;
    return p;
  }
  if (f.M <= 0 || f.N <= 0) return p;
  p.group_m = k.group > 0 ? k.group : PSO_GEMM_GROUP_M;
  // staged 16-B epilogue for bf16 outputs with 16-B aligned rows (5-10 % on the K = 640 / 1280 projections with
  // bias + residual, tools/epi_bench.py); variant 41 keeps the per-lane 8-B epilogue (A/B knob)
  const bool rows16 = f.out_dtype != PSO_F32 && f.out16 && f.ldo8 && f.resid16;  // 16-bit out (+ resid) in 16-B rows
  p.stage_epi = gv_raw != PSO_GV_LANE_EPILOGUE && rows16;
  p.vec_ok = f.ldo4 && f.out_vec && f.resid8 && f.bias8 && f.rowbias8 && f.ld_rowbias4;
  const bool bn64_only = f.tail_group_n > 0 && (f.tail_group_n % 128) != 0;  // grouped tail needs BN | group
  const bool bn256_ok = f.tail_group_n == 0 || (f.tail_group_n % 256) == 0;
  const long Ktot = (long)f.K1 + (f.has_tail ? f.K2 : 0);
  auto tiles = [&](int bm, int bn) { return (long)((f.M + bm - 1) / bm) * ((f.N + bn - 1) / bn); };
  if (f.batch > 1) {  // batched dense product (the VAE's single-head mid attention): the 2-phase tiles only
    if ((f.N % 160) == 0 && tiles(128, 160) * f.batch >= 256) return plan_tile(p, 128, 160, 2, 2, 2);
    if (tiles(128, 128) * f.batch >= 256) return plan_tile(p, 128, 128, 2, 4, 2);
    return plan_tile(p, 64, 64);
  }
  // deterministic split-K through the caller's workspace (pso_gemm_ws / pso_conv2d_ws): small M x N, long K; applies
  // when the plan splits and the caller's workspace holds every split
  if (f.have_ws && gemm_ws_allowed(k)) {
    const SplitPlan sp = gemm_split_plan(f.M, f.N, f.K1, f.K2, f.has_tail, k);
    if (sp.ks >= 2 && f.ws_bytes >= (size_t)sp.ks * f.M * f.N * sizeof(float) && f.ldo4 && f.out_vec &&
        (f.tail_group_n % sp.bn) == 0 && (!f.conv_mode || (f.resid8 && f.ld_rowbias4))) {
      p.ws_ks = sp.ks;
      return sp.bn == 160 ? plan_tile(p, 128, 160, 2, 2, 2) : plan_tile(p, 128, 128, 2, 4, 2);
    }
  }
  const bool no_epi_operands = !f.has_bias && !f.has_rowbias && !f.has_resid;
  // Skinny N (the LoRA rank-r products): one 16-row x all-N tile per 4-wave block, K split over the waves.
  if (gv == 0 && !f.conv_mode && !f.has_tail && no_epi_operands && f.N <= 128 && (f.N % 4) == 0 && p.vec_ok &&
      f.M >= 256) {
    p.form = GF_SKINNY;
    return p;
  }
  // Small outputs with a long reduction: split K over blocks, f32 atomics in the epilogue.
  const bool can_split = f.out_dtype == PSO_F32 && f.accumulate && no_epi_operands && !f.conv_mode &&
                         f.tail_group_n == 0;
  if (can_split && (f.M <= 128 || f.N <= 128) && Ktot >= 2048) {
    const long ktiles = (Ktot + 64 - 1) / 64;
    long ks = (512 + tiles(64, 64) - 1) / tiles(64, 64);
    if (ks > ktiles / 2) ks = ktiles / 2;
    if (ks < 1) ks = 1;
    p.atomic_ks = (int)ks;
    return plan_tile(p, 64, 64);
  }
  // the 256 x 320 8-phase forms want three quarters of a round of tiles: that already beats the 2-phase tiles (C4's
  // 12288 x 1280 x 5120: 1072 vs 811 TF/s, x 1280: 875 vs 830; C3's 24576 x 640 x 2560: 1034 vs 725, x 640: 685 vs
  // 612 -- 192 tiles each); half a round does not (8192 x 1280 x 1280: 574 vs 776).  Variant 46 / 47 keep the
  // full-round rule.
  const long min320 = (gv_raw == PSO_GV_ROUND2_RULES || gv_raw == PSO_GV_8P320_FULL_ROUND) ? 256 : 192;
  // 3x3 / stride 1 / pad 1 convolutions (the ResNet convs and their input gradients) on the 8-phase 256 x 320 tiles
  // (gemm8p.hip CONV form) wherever they fill a round of CUs; variant 43 keeps them on the 2-phase kernel, 44 forces it
  {
    const long hw = (long)f.Ho * f.Wo;
    const bool conv8 = conv3x3_same && (f.C1 % 64) == 0 && f.C1 <= 4096 && (hw % 256) == 0 &&
                       (f.H & (f.H - 1)) == 0 && (f.W & (f.W - 1)) == 0 && f.W >= 8 && (f.N % 320) == 0 && rows16 &&
                       f.bias8 && f.rowbias8 && (!f.has_rowbias || f.rowgroup_hw) && f.fits_conv && f.fits_b && f.ab16;
    const long t320c = (long)(f.M / 256) * (f.N / 320);
    if (conv8 && gv_raw != PSO_GV_CONV8_OFF && (gv_raw == PSO_GV_FORCE_CONV8 || (gv == 0 && t320c >= min320)))
      return plan_8p(p, GF_8P320_CONV, 320);
  }
  // 8-phase 256x256 (gemm8p.hip, wave groups staggered) for dense bf16 GEMMs with N % 256 == 0: LDS-staged 16-B
  // epilogue, LoRA K-tail, bias / alpha / residual.  Default for N >= 2560 with >= 256 tiles (tools/gemm8_ab.py, one
  // box: q/k/v 16384 x 3840 x 1280 1071 vs 937 TF/s, ff.out dX 8192 x 5120 x 1280 991 vs 945); N = 1280 keeps 128x160
  // (1.25 rounds of 256x256 tiles at M = 16384: 805 vs 928).  Variant 30 forces it, 31 keeps it off everywhere.
  const bool base8 = !f.conv_mode && !f.has_rowbias && !f.accumulate && (f.K1 % 64) == 0 && f.ab16 && f.ld_ab8 &&
                     rows16 && f.bias8 && f.fits_a && f.fits_b && (!f.has_tail || f.fits_tail);
  auto tail_groups_of = [&](int bn) { return !f.has_tail || f.tail_group_n == 0 || (f.tail_group_n % bn) == 0; };
  const bool ok8 = base8 && (f.N % 256) == 0 && tail_groups_of(256);
  const long t256 = (long)((f.M + 255) / 256) * (f.N / 256);
  // 8-phase 256 x 320 (gemm8p.hip): every SDXL width is a multiple of 320, and at the UNet's M (256 * 2^k rows) the
  // tile count is a whole number of 256-CU rounds (N = 1280 at M = 16384: 256 tiles; N = 640 at M = 65536: 512).
  // Default where it fills at least one round and the reduction is short (K < 2560: the 256 x 160 persistent form
  // keeps the long ones); at half a round (M = 8192, N = 1280: 128 tiles) the 2-phase 128 x 160 stays ahead
  // (tools/shape_prof.py, one box: 16384 x 1280 x 1280 + LoRA 922 vs 816 TF/s, 65536 x 640 x 640 + LoRA 700 vs 652,
  // 65536 x 1920 x 640 + LoRA 849 vs 783; 8192 x 1280 x 1280 + LoRA 574 vs 776).  Variant 39 forces it, 40 keeps it
  // off.
  const bool ok320 = base8 && (f.N % 320) == 0 && f.ld_ab_eq && (!f.has_tail || f.K2 <= 64) && tail_groups_of(320);
  const long t320 = (f.N % 320) == 0 ? (long)((f.M + 255) / 256) * (f.N / 320) : 0;
  // wide N (>= 2560) whose 256 x 256 tiles leave a partial round while the 256 x 320 ones make whole rounds (C3's
  // 6144 x 10240 x 1280: 960 vs 768 tiles, 979 vs 1079 TF/s; 24576 x 5120 x 640: 802 vs 832) take the 320 form below;
  // variant 46 keeps the round-2 rules
  const bool wide320 = gv == 0 && gv_raw != PSO_GV_ROUND2_RULES && ok320 && f.N >= 2560 && (t256 % 256) != 0 &&
                       t320 >= 256 && (t320 % 256) == 0;
  // three quarters of a round of 256 x 256 tiles where the 256 x 320 ones leave more CUs idle (C4's 12288 x 1280:
  // 240 vs 192 tiles, 1056 vs 877-919 TF/s; bs = 1's q/k/v 4096 x 3840: 240 tiles, 938 vs 798 on the 2-phase
  // tiles; tools/small_m_bench.py); variant 50 keeps the full-round rule
  const bool part256 = gv == 0 && gv_raw != PSO_GV_8P256_FULL_ROUND && t256 >= 192 && t256 < 256 && t256 > t320;
  if (ok8 && !wide320 &&
      (gv == PSO_GV_FORCE_8P256 || part256 ||
       ((gv == PSO_GV_8P256_ANY_N || (gv == 0 && f.N >= 2560)) && t256 >= 256)))
    return plan_8p(p, GF_8P256, 256);
  if (ok320 && gv_raw != PSO_GV_8P320_OFF && gv_raw != PSO_GV_FORCE_8P160 &&
      (gv_raw == PSO_GV_FORCE_8P320 || wide320 ||
       (gv == 0 && t320 >= min320 && f.N < 2560 && (gv_raw != PSO_GV_8P320_SHORT_K || Ktot < 2560))))
    return plan_8p(p, GF_8P320, 320);
  // 8-phase 256 x 160 (gemm8p.hip) for the N % 160 == 0 widths with at least one round of tiles and a long reduction
  // (K >= 2560: ff.out 16384 x 1280 x 5120 972 vs 942 TF/s, 32768 x 640 x 5120 1039 vs 910, 65536 x 640 x 2560 823
  // vs 770); at K = 640 / 1280 the 2-phase 128 x 160 with two co-resident blocks per CU (one block's epilogue beside
  // the other's main loop) stays ahead (16384 x 1280 x 1280 827 vs 724, tools/shape_prof.py one box).  Variant 37
  // keeps the 2-phase 128 x 160, 38 forces the 8-phase form wherever it applies.
  const bool ok160 = base8 && (f.N % 160) == 0 && tail_groups_of(160);
  const long t160 = (long)((f.M + 255) / 256) * (f.N / 160);
  if (ok160 && gv_raw != PSO_GV_8P160_OFF &&
      (gv_raw == PSO_GV_FORCE_8P160 || (gv == 0 && t160 >= 256 && Ktot >= 2560)))
    return plan_8p(p, GF_8P160, 160);
  const bool n160 = (f.N % 160) == 0 && (f.tail_group_n == 0 || (f.tail_group_n % 160) == 0);
  const bool n320 = (f.N % 320) == 0 && (f.tail_group_n == 0 || (f.tail_group_n % 320) == 0);
  const bool n80 = (f.N % 80) == 0 && (f.tail_group_n % 80) == 0;
#define PSO_PLAN_FORCED(V, OK, BM, BN, WM, WN, ST, PIPE) \
  if (gv == V && (OK)) return plan_tile(p, BM, BN, WM, WN, ST, PIPE);
  PSO_FORCED_TILES(PSO_PLAN_FORCED)
#undef PSO_PLAN_FORCED
  // Tile choice by occupancy (~2 co-resident 4-wave blocks per CU, 256 CUs): large grids keep 128x128 (best operand
  // reuse); grids that would leave CUs idle drop to 64x128 / 128x64 / 64x64 (e.g. the L2 projections, M=4096 N=1280,
  // and the skinny LoRA projections N = r..3r).
  if (f.N <= 64) return plan_tile(p, 64, 64);
  if (bn64_only) return tiles(128, 64) >= 512 ? plan_tile(p, 128, 64) : plan_tile(p, 64, 64);
  if (f.M <= 64) return plan_tile(p, 64, 128);
  // 256x256 block tile, 8 waves x (128x64): twice the MFMAs per LDS fragment read; wins once the grid covers the 256
  // CUs (one 128 KiB-LDS block per CU) and N has no partial 256-column tile; implicit-GEMM convs (long K) already
  // at half a wave of blocks.  Otherwise 128x128 with 8 waves (64x32 each).  Measured on the UNet shapes at 8 images
  // (tools/gemm_bench.py): e.g. L2 qkv 8192x3840x1280 713 vs 645 TF/s; L2 proj 8192x1280x1280 531 vs 474.
  // Very large grids (>= 4 rounds of 256x256 tiles: L1/L2 ff.proj, the 128^2 upsample conv) keep 256x256.  Otherwise
  // N % 160 == 0 (every SDXL width: 320 | N) takes 128x160 with 4 waves of 64x80: fewer LDS bytes per MFMA than the
  // 8-wave 128x128 (64x32 wave tiles) and tile counts that divide the 512 co-resident slots (M=8192, N=1280 -> 512
  // tiles).  tools/gemm_bench.py at 8 images: L2 ff.out 8192x1280x5120 797 -> 1097 TF/s, L2 proj 636 -> 816,
  // L0/L1/L2 3x3 convs 733/887/795 -> 921/994/1005.
  if (bn256_ok && (f.N % 256) == 0 && tiles(256, 256) >= 1024) return plan_tile(p, 256, 256, 2, 4, 2);
  // 128 x 160 tiles that leave a quarter of the 512 co-resident slots empty while 128 x 128 ones nearly fill them
  // (C3's 6144-row L2 products, N = 1280: 384 vs 480 tiles; proj 678 -> 753 TF/s, ff.out 860 -> 971, GEGLU dX
  // 940 -> 1023, 3x3 conv 802 -> 864): the 8-wave 128 x 128 kernel.  At half the slots (4096 x 1280, the bs=1 LoRA
  // pass: 256 vs 320 tiles) 128 x 160 stays ahead (step 90.5 vs 93.2 ms).  Variant 46 keeps the 128 x 160 choice.
  if (gv_raw != PSO_GV_ROUND2_RULES && !bn64_only && n160 && tiles(128, 160) >= 384 && tiles(128, 160) < 512 &&
      tiles(128, 128) <= 512)
    return plan_tile(p, 128, 128, 2, 4, 2);
  // 128 x 160 tiles that make at most one workgroup per CU while 64 x 160 ones make 1.5-2 (the bs = 1 / GPU pass:
  // 4096 x 1280 and 8192 x 640 rows; tools/small_m_bench.py, one box: 4096 x 1280 x 5120 837 vs 755 TF/s, x 1280 + LoRA
  // 649 vs 540, 8192 x 640 x 5120 843 vs 759, x 1920 + LoRA 718 vs 637); variant 48 keeps 128 x 160 there
  if (gv_raw != PSO_GV_KEEP_T128x160 && n160 && tiles(128, 160) <= 256 && tiles(64, 160) >= 384)
    return plan_tile(p, 64, 160, 2, 2, 2);
  // smaller still (M = 2048, N = 1280: 256 tiles of 64 x 160, 640 of 64 x 64), short K (the long ones split K through
  // a workspace, pso_gemm_ws): variant 49 takes the register-pipelined 8-wave 128 x 128 tiles. They win in isolation
  // (tools/small_m_bench.py: 2048 x 1280 x 1280 + LoRA 404 vs 319 TF/s) but lose inside the bs = 1 step
  // (tools/shape_prof.py, one box: 252-256 vs 277 TF/s), so 64 x 64 stays the default there
  if (gv_raw == PSO_GV_SMALL_M_T128x128_P && !f.conv_mode && !bn64_only && (f.N % 128) == 0 &&
      tiles(64, 160) <= 256 && tiles(128, 128) >= 128 && tiles(128, 160) < 256)
    return plan_tile(p, 128, 128, 2, 4, 2, true);
  if (n160 && tiles(128, 160) >= 256) return plan_tile(p, 128, 160, 2, 2, 2);
  if (bn256_ok && (f.N % 256) == 0 && tiles(256, 256) >= (f.conv_mode ? 128 : 256))
    return plan_tile(p, 256, 256, 2, 4, 2);
  if (tiles(128, 128) >= 256) return plan_tile(p, 128, 128, 2, 4, 2);
  if (tiles(64, 128) >= 512) return (f.N % 128 == 0) ? plan_tile(p, 64, 128) : plan_tile(p, 128, 64);
  return plan_tile(p, 64, 64);
}

// GEGLU forward (pso_gemm_geglu: N = 2 F interleaved columns, N % 256 == 0): 8-phase wherever K % 64 == 0
constexpr GemmPlan geglu_plan(int M, int N, int K, bool ld_ab_eq, bool fits, const GemmKnobs& k) {
  GemmPlan p;
  p.epi = GEPI_GEGLU;
  p.vec_ok = true;
  p.group_m = k.group > 0 ? k.group : PSO_GEMM_GROUP_M;
  const int v = k.variant;
  const bool ok8 = v != PSO_GV_NO_8P && (K % 64) == 0 && fits;
  // the 8-phase kernel with the LDS-staged epilogue (gemm8p.hip): 16384 x 10240 x 1280 1023 vs 801 TF/s,
  // 65536 x 5120 x 640 814 vs 640 (tools/gemm_bench.py, one box), inside the C2 step 1006 vs 922 / 801 vs 706
  // (tools/shape_prof.py); variant 31 keeps the 2-phase 256x256 kernel
  // 256 x 320 tiles where they cost fewer tile-rounds than 256 x 256 (rounds x tile width: bs = 1's 4096 x 10240:
  // 2 x 320 < 3 x 256; C3's 6144 x 10240: 3 x 320 < 4 x 256; C5's 2048 x 10240: 1 x 320 < 2 x 256; equal at C2's
  // whole-round shapes, which keep 256 x 256); same bits either way.  Variant 57 keeps 256 x 256.
  if (ok8 && v != PSO_GV_GEGLU_KEEP_256 && (N % 320) == 0 && ld_ab_eq) {
    const long r256 = ((long)((M + 255) / 256) * (N / 256) + 255) / 256, r320 = ((long)((M + 255) / 256) * (N / 320) + 255) / 256;
    // variant 58 (knob): 256 x 320 at equal rounds too (C2's shapes)
    if (r320 * 320 < r256 * 256 || (v == PSO_GV_GEGLU_320_EQUAL && r320 * 320 == r256 * 256))
      return plan_8p(p, GF_8P320, 320);
  }
  if (ok8) return plan_8p(p, GF_8P256, 256);
  // tile A/B knobs (64-column wave tiles are what the interleaved epilogue needs)
  if (v == PSO_GV_GEGLU_T128x128) return plan_tile(p, 128, 128, 2, 2, 2);
  if (v == PSO_GV_GEGLU_T128x256) return plan_tile(p, 128, 256, 2, 4, 2);
  if (v == PSO_GV_GEGLU_T256x128_4x2) return plan_tile(p, 256, 128, 4, 2, 2);
  if (v == PSO_GV_GEGLU_T128x128_S3) return plan_tile(p, 128, 128, 2, 2, 3);
  return plan_tile(p, 256, 256, 2, 4, 2);
}

// GEGLU backward (pso_gemm_geglu_bwd: N = F columns of dout, N % 32 == 0)
constexpr GemmPlan geglu_bwd_plan(int M, int N, int K, bool ld_ab_eq, bool fits, const GemmKnobs& k) {
  GemmPlan p;
  p.epi = GEPI_GEGLU_BWD;
  p.vec_ok = true;
  p.group_m = k.group > 0 ? k.group : PSO_GEMM_GROUP_M;
  const bool ok8 = k.variant != PSO_GV_NO_8P && (K % 64) == 0 && fits;
  // 256 x 320 tiles where they make whole rounds the 256 x 256 ones do not (8192 x 5120: 512 tiles = 2 rounds vs 640 =
  // 2.5; 32768 x 2560: 1024 = 4 vs 1280 = 5); variant 45 keeps the 256 x 256 form
  if (ok8 && k.variant != PSO_GV_GEGLU_BWD_320_OFF && (N % 320) == 0 && ld_ab_eq &&
      ((long)((M + 255) / 256) * (N / 320)) % 256 == 0)
    return plan_8p(p, GF_8P320, 320);
  // 8-phase form (staggered wave groups) by default: 716 vs 658 TF/s for the 2-phase 128x160 kernel at
  // 16384 x 5120 x 1280, 489 vs 472 at 65536 x 2560 x 640 (tools/gemm_bench.py, one box); variant 31 keeps 128x160
  // (from two rounds of tiles: below that the 2-phase 128 x 160 tiles with two workgroups per CU win -- bs = 1's
  // 2048 x 5120 x 1280 620 vs 493-522 TF/s, C3's 6144 x 5120 x 1280 719 vs 680; tools/small_m_bench.py GEGLU_BWD=1)
  if (ok8 && (N % 256) == 0 && (long)((M + 255) / 256) * (N / 256) >= 512) return plan_8p(p, GF_8P256, 256);
  const long t160 = (long)((M + 127) / 128) * ((N + 159) / 160);
  if ((N % 160) == 0 && t160 >= 256) return plan_tile(p, 128, 160, 2, 2, 2);
  return plan_tile(p, 64, 64, 2, 2, 2);
}

// =====================================================================================================================
// TN products: out[I][J] += alpha * sum_m A[m][I] * B[m][J]
// =====================================================================================================================
//   TNP_RANK:  one side a rank-16/32/64/96 projection -> the rank-r streaming kernel (gemm_tn_rank.hip)
//   TNP_256:   both sides multiples of 256 -> 256 x 256 tiles: alone, or one round of workspace slices where the tiles
//              are too few for the CUs
//   TNP_128:   both sides >= 128 wide -> 128 x 128 tiles, ks slices (workspace: the small-weight split of
//              tn_ws_slices, else the split the atomic form takes)
//   TNP_64:    the rest -> 64 x 64 tiles, ks slices
//   TNP_BAD_GROUP: a grouped product without a rank-r side (an argument error)
// ws: every split of the reduction rows stores its partial product into the caller's workspace and the partials are
// added in split order -- no f32 atomics anywhere; else splits (ks > 1) add with f32 atomics.
enum TnKind { TNP_RANK = 1, TNP_128 = 2, TNP_64 = 3, TNP_256 = 4, TNP_BAD_GROUP = 5 };
struct TnPlan {
  int kind = TNP_64;
  bool ws = false;
  int ks = 1, steps = 0;  // slices of the reduction rows; 64-row K-steps per slice (TNP_128 / TNP_256)
  bool swap = false;      // TNP_RANK: the rank-r side is A (I), the wide one B
  int rank = 0;           // TNP_RANK: r (per group)
};
constexpr bool tn_rank_ok(int r) { return r == 16 || r == 32 || r == 64 || r == 96; }
constexpr bool tn_fits(int M, long lda, long ldb) { return (long)M * lda < (1L << 30) && (long)M * ldb < (1L << 30); }

// the 256 x 256 TN tiles (variant 56 keeps the 128 x 128 ones): both sides multiples of 256 and the operands within
// 32-bit buffer offsets.  Returns the slice count: 1 where the tiles alone cover >= 3/4 of the CUs (out += directly);
// one round of workspace slices of >= 8 K-steps each where the 128 x 128 tiles would run one pass of 256-383
// workgroups (< 3/4 of the two-per-CU slots, and too many for tn_ws_slices); else 0 = not this kernel.
// tools/tn_full_bench.py, TF/s 256 vs 128 tiles: 6144 x 1280 x 11520 (225 tiles) 948 / 929 vs 835 / 836, 24576 x 1280
// x 11520 990 vs 823, the GEGLU 6144 x 10240 x 1280 (200 tiles) 720 / 736 vs 658 / 725, 6144 x 3840 x 1280 (75 tiles x
// 3 slices) 675 / 683 vs 607 / 616; slices where the 128 x 128 tiles already fill the slots lose (6144 x 1280 x 5120,
// 100 tiles x 2: 670 vs 752; 6144 x 1280 x 1280, 25 x 10: 411 vs 471): the partials' round trip through HBM.
constexpr int tn256_slices(int M, int I, int J, long lda, long ldb, const GemmKnobs& k) {
  if (k.variant == PSO_GV_TN256_OFF || I % 256 || J % 256 || !tn_fits(M, lda, ldb)) return 0;
  const int t256 = (I / 256) * (J / 256);
  if (t256 >= 192) return 1;
  const int t128 = (I / 128) * (J / 128);
  if (t128 < 256 || t128 >= 384) return 0;
  const int nkt = (M + 63) / 64;
  int ks = 256 / t256;
  if (ks > nkt / 8) ks = nkt / 8;
  if (ks < 2) return 0;
  const int steps = (nkt + ks - 1) / ks;
  return (nkt + steps - 1) / steps;
}

// split of the full-weight TN product into ks slices of the reduction rows for the workspace form: enough slices for
// ~1.5 rounds of 128 x 128 tiles over the 256 CUs, each slice >= 8 K-steps (512 rows)
constexpr int tn_ws_slices(int M, int I, int J) {
  if (I < 128 || J < 128) return 0;
  const int t128 = ((I + 127) / 128) * ((J + 127) / 128);
  if (t128 >= 256) return 0;
  const int nkt = (M + 63) / 64;
  int ks = (384 + t128 - 1) / t128;
  if (ks > nkt / 8) ks = nkt / 8;
  return ks >= 2 ? ks : 0;
}

// the split of the 128 x 128 tiles over M with f32 atomics: only as far as needed to cover ~2 rounds of co-resident
// blocks, and only while its f32 atomics stay small next to the product: each split adds I*J*4 bytes at the
// ~1.3 TB/s atomic rate against 2*M*I*J flop, so ks <= M / 16384 keeps them under ~10 %.
// Returns 0 below 128 blocks (e.g. 640 x 640 weights: 25 tiles), which leave most CUs idle: the 64 x 64 kernel's 4x the
// tiles win there (C3 step shape_prof: 24576 x 640 x 640 122 vs 59 TF/s, 6144 x 1280 x 1280 234 vs 213; the 128 x 128
// tiles elsewhere: 6144 x 10240 x 1280 697 vs 417, 98304 x 320 x 2880 485 vs 141, 6144 x 1280 x 11520 815 vs 431)
constexpr int tn128_atomic_slices(int M, int I, int J) {
  const int nkt = (M + 63) / 64;
  const int t128 = ((I + 127) / 128) * ((J + 127) / 128);
  int ks = (512 + t128 - 1) / t128;
  if (ks > M / 16384) ks = M / 16384;
  if (ks < 1) ks = 1;
  const int steps = (nkt + ks - 1) / ks;
  ks = (nkt + steps - 1) / steps;
  return t128 * ks >= 128 ? ks : 0;
}

// group > 0 (block-diagonal fused q/k/v, rank-r kernel only): the big side's column c pairs with the small side's
// columns [(c / group) * r, +r) where r = small width / (big / group).  have_ws: a usable workspace was supplied
// (pso_gemm_tn_ws); the plan then says whether it is used (ws).  M > 0; I, J multiples of 8.
constexpr TnPlan tn_plan(int M, int I, int J, long lda, long ldb, int group, bool have_ws, const GemmKnobs& k) {
  TnPlan p;
  const int nkt = (M + 63) / 64;
  const bool autosplit = k.tn_split == 0;
  const auto slices = [&](int kind, int ks, bool ws) {  // ks slices of whole K-steps
    p.kind = kind; p.ws = ws;
    p.steps = (nkt + ks - 1) / ks;
    p.ks = (nkt + p.steps - 1) / p.steps;
    return p;
  };
  if (autosplit) {  // one side a rank-r projection (LoRA): the streaming rank kernel
    p.ws = have_ws;
    p.kind = TNP_RANK;
    if (I % 128 == 0 && (group == 0 ? tn_rank_ok(J) : (group % 128 == 0 && I % group == 0 && tn_rank_ok(J / (I / group))))) {
      p.rank = group ? J / (I / group) : J;
      return p;
    }
    if (J % 128 == 0 && group == 0 && tn_rank_ok(I)) {
      p.swap = true; p.rank = I;
      return p;
    }
    p.ws = false;
  }
  if (group != 0) {
    p.kind = TNP_BAD_GROUP;
    return p;
  }
  const int ks256 = autosplit ? tn256_slices(M, I, J, lda, ldb, k) : 0;
  if (ks256 == 1 || (ks256 >= 2 && have_ws)) return slices(TNP_256, ks256, ks256 >= 2);
  if (autosplit && I >= 128 && J >= 128 && tn_fits(M, lda, ldb)) {
    // full-weight gradients (both sides >= 128 wide): 128 x 128 tiles
    const int ks_ws = have_ws ? tn_ws_slices(M, I, J) : 0;
    const int ks = ks_ws ? ks_ws : tn128_atomic_slices(M, I, J);
    const bool ws = have_ws && ks >= 2;
    if (ks >= 1 && (ws || !k.tn128_off)) return slices(TNP_128, ks, ws);
  }
  // ~160 blocks: fewer leaves the M-range latency-bound, more multiplies the f32 atomics (measured optimum on the
  // LoRA dW shapes, M = 4096 / 16384, I x J = 1280x32 .. 640x32)
  const int tiles = ((I + 63) / 64) * ((J + 63) / 64);
  int ks = autosplit ? (160 + tiles - 1) / tiles : k.tn_split;
  if (ks > nkt) ks = nkt;
  if (ks < 1) ks = 1;
  p.kind = TNP_64;
  p.ks = ks;
  p.ws = have_ws && autosplit && ks >= 2;
  return p;
}

// pso_gemm_tn_geglu (I = F2, a multiple of 128; J >= 128): one pass over the reduction rows (no split: += straight
// into the natural-order gradient, deterministic) on the 256 x 256 tiles where the plan takes them alone, else on
// the 128 x 128 ones; the split knob does not apply
constexpr TnPlan tn_geglu_plan(int M, int F2, int J, long lda, long ldb, const GemmKnobs& k) {
  GemmKnobs k0 = k;
  k0.tn_split = 0;
  TnPlan p;
  p.kind = tn_plan(M, F2, J, lda, ldb, 0, false, k0).kind == TNP_256 ? TNP_256 : TNP_128;
  p.steps = (M + 63) / 64;
  return p;
}

#endif  // PSO_GEMM_PLAN_H
