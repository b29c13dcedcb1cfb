// bf16 MFMA GEMM / implicit-GEMM convolution for gfx950 (CDNA4), fp32 accumulate.
//
//   out[M][N] = epilogue( alpha * ( A1[M][K1] . B1[N][K1]^T  +  A2[M][K2] . B2[N][K2]^T ) )
//   epilogue  = + bias[N] + rowbias[m / rows_per_group][N] + resid[M][N]   -> bf16 | f32 | f32 accumulate
//
// Replaces the implicit cuBLAS GEMMs (every nn.Linear of the SDXL UNet / VAE and the peft LoRA product, SURVEY §2
// "cuBLAS GEMM") and the cuDNN conv2d (SURVEY §2 "cuDNN conv2d"): the conv is an implicit GEMM whose A operand is
// gathered on the fly from an NHWC image (M = B*Ho*Wo pixels, K = kh*kw*Cin), with three gather modes:
//   NORMAL  iy = oy*S + kh - P        (conv 3x3/1x1, stride 1 or 2)
//   UP2     iy = (oy + kh - P) >> 1   (nearest 2x upsample fused into the following conv, diffusers Upsample2D)
//   T2      iy = (oy + P - kh) / 2    (transposed stride-2 conv: input-gradient of the Downsample2D conv)
// and an optional second channel source (torch.cat([h, skip], dim=1) of the up blocks, fused into the gather).
// The second (A2, B2) operand pair is the LoRA up-projection fused as a K-tail: y = x W^T + (x A^T)(s B)^T.
//
// Tiling: 256 threads = 4 waves (2 x 2), block tile BM x BN x 64, wave tile (BM/2) x (BN/2) built from
// v_mfma_f32_16x16x32_bf16.  Operands are staged global -> VGPR -> LDS (double buffered, one barrier per K-tile) with
// an XOR swizzle (chunk ^ (row & 7)) that makes both the ds_write_b128 and the ds_read_b128 fragment reads
// conflict-free on 128-B rows.  The MFMA is issued with the B (weight) fragment first so that every lane ends up
// holding 4 consecutive output columns of one row -> 8-B / 16-B vector epilogue stores.
//
// Which kernel runs is decided in gemm_plan.h (facts -> plan, plain host C++); this file fills the facts, launches what
// the plan says, and holds the device code of the 2-phase tiles and the TN kernels.
#include "gemm_args.h"
#include "gemm_plan.h"

#include <cstdlib>

#define GEMM_THREADS 256
#define BK 64

#define EPI_NONE 0
#define EPI_GEGLU 1
#define EPI_GEGLU_BWD 2

__device__ __forceinline__ int swz(int r, int c) { return r * BK + ((c ^ (r & 7)) << 3); }

template <int BM, int BN, int WAVES>
struct Tile {
  // 8-row x 128-B glds pieces per K-tile (A_P, B_P) and per wave (A_CH, B_CH).  When WAVES does not divide a count
  // (BN = 160 over 8 waves: 20 pieces), wave w takes pieces w, w + WAVES, ... and the waves left short repeat the last
  // piece (same source, same bytes, same LDS slot), so every wave issues the same number of loads: counted vmcnt waits
  // stay uniform.
  static constexpr int A_P = BM / 8, B_P = BN / 8;
  static constexpr int A_CH = (A_P + WAVES - 1) / WAVES;
  static constexpr int B_CH = (B_P + WAVES - 1) / WAVES;
  static constexpr bool A_EVEN = A_P % WAVES == 0, B_EVEN = B_P % WAVES == 0;
};

// ---- per-row conv coordinates (precomputed once per thread) ----
struct RowCoord {
  int b, oy, ox;
  bool valid;
};

__device__ __forceinline__ uint4 load_chunk_dense(const bf16_t* p, long ld, int row, int nrows, int k, int K) {
  if (row < nrows && k < K) return *reinterpret_cast<const uint4*>(p + (long)row * ld + k);
  return make_uint4(0, 0, 0, 0);
}

// per-K-tile conv gather state (uniform over the tile: BK divides every channel source, so one tap / source)
struct TapInfo {
  int kh, kw;
  int c0;            // channel offset inside the selected source
  int Cs;            // channel count (row pitch) of the selected source
  const bf16_t* src;
  bool valid;
};

__device__ __forceinline__ TapInfo tap_info(const GemmArgs& g, int k0) {
  const ConvGeom& cv = g.conv;
  const int Ct = cv.C1 + cv.C2;
  TapInfo t;
  t.valid = k0 < g.K1;
  const int tap = k0 / Ct;
  const int c = k0 - tap * Ct;
  t.kh = tap / cv.ks;
  t.kw = tap - t.kh * cv.ks;
  if (c < cv.C1) { t.src = g.a1; t.c0 = c; t.Cs = cv.C1; }
  else { t.src = cv.src2; t.c0 = c - cv.C1; t.Cs = cv.C2; }
  return t;
}

template <int MODE>
__device__ __forceinline__ uint4 load_chunk_conv(const ConvGeom& cv, const TapInfo& t, const RowCoord& rc, int kc) {
  if (!rc.valid || !t.valid) return make_uint4(0, 0, 0, 0);
  int iy, ix;
  if (MODE == PSO_CONV_NORMAL) {
    iy = rc.oy * cv.stride + t.kh - cv.pad;
    ix = rc.ox * cv.stride + t.kw - cv.pad;
    if ((unsigned)iy >= (unsigned)cv.H || (unsigned)ix >= (unsigned)cv.W) return make_uint4(0, 0, 0, 0);
  } else if (MODE == PSO_CONV_UP2) {
    const int uy = rc.oy + t.kh - cv.pad, ux = rc.ox + t.kw - cv.pad;
    if ((unsigned)uy >= (unsigned)(2 * cv.H) || (unsigned)ux >= (unsigned)(2 * cv.W)) return make_uint4(0, 0, 0, 0);
    iy = uy >> 1;
    ix = ux >> 1;
  } else {  // T2
    const int ty = rc.oy + cv.pad - t.kh, tx = rc.ox + cv.pad - t.kw;
    if (ty < 0 || tx < 0 || (ty & 1) || (tx & 1)) return make_uint4(0, 0, 0, 0);
    iy = ty >> 1;
    ix = tx >> 1;
    if (iy >= cv.H || ix >= cv.W) return make_uint4(0, 0, 0, 0);
  }
  const long pix = ((long)rc.b * cv.H + iy) * cv.W + ix;
  return *reinterpret_cast<const uint4*>(t.src + pix * t.Cs + t.c0 + kc);
}

__device__ __attribute__((aligned(16))) uint4 g_zero16[4];  // source of every zero-filled (padding / tail) chunk

typedef __attribute__((address_space(3))) void lds_void;

// s_waitcnt the compiler's waitcnt pass can see (inline asm is opaque to it).  The builtin exists only in the device
// compilation; the host pass must not see it or the kernel stubs are silently dropped.
#if defined(__HIP_DEVICE_COMPILE__)
#define PSO_S_WAITCNT(imm) __builtin_amdgcn_s_waitcnt(imm)
#else
#define PSO_S_WAITCNT(imm) ((void)0)
#endif

// Wait until at most n K-tiles' worth of this wave's direct-to-LDS loads (P pieces each) are still in flight (n is
// wave-uniform, 0..3: the STAGES <= 5 rings), then the block barrier; LGKM also retires this wave's LDS reads first.
template <int P, bool LGKM>
__device__ __forceinline__ void vm_wait_barrier(int n) {
  static_assert(3 * P <= 63, "vmcnt field");
  if (n >= 3) {
    if (LGKM) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(3 * P) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(3 * P) : "memory");
  } else if (n == 2) {
    if (LGKM) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(2 * P) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(2 * P) : "memory");
  } else if (n == 1) {
    if (LGKM) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(P) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(P) : "memory");
  } else {
    if (LGKM) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
  }
}

// Direct-to-LDS staging (global_load_lds_dwordx4): wave w fills 8-row x 128-B pieces; lane i of a piece lands at
// byte 16*i of it (row i/8, physical chunk i%8), so the XOR swizzle is applied to the SOURCE chunk: physical chunk p of
// row R holds logical chunk p ^ (R & 7) -- the same involution swz() applies on the read side.
// WM x WN waves, each owning a (BM/WM) x (BN/WN) accumulator tile; STAGES-deep LDS ring with STAGES-1 K-tiles of
// direct-to-LDS loads in flight behind a counted vmcnt and a raw s_barrier (a __syncthreads() would drain them).
template <int BM, int BN, int CONV, int WM, int WN, int STAGES, bool PIPE = false, int EPI = EPI_NONE>
__global__ __launch_bounds__(64 * WM * WN, 1) void gemm_bf16_kernel(GemmArgs g) {
  constexpr int WAVES = WM * WN;
  using T = Tile<BM, BN, WAVES>;
  constexpr int MI = BM / WM / 16;  // 16-row subtiles per wave
  constexpr int NJ = BN / WN / 16;  // 16-col subtiles per wave
  constexpr int PIECES = T::A_CH + T::B_CH;  // glds per wave per K-tile
  static_assert(BM % 8 == 0 && BN % 8 == 0, "tile / wave split");
  extern __shared__ __attribute__((aligned(16))) bf16_t lds_dyn[];
  bf16_t* lds_base = lds_dyn;
  auto stage_ptr = [&](int s) { return lds_base + s * (BM + BN) * BK; };

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave - (wave / WN) * WN;
  auto pa = [&](int i) { return T::A_EVEN ? wave * T::A_CH + i : min(wave + WAVES * i, T::A_P - 1); };
  auto pb = [&](int i) { return T::B_EVEN ? wave * T::B_CH + i : min(wave + WAVES * i, T::B_P - 1); };

  // XCD-aware block order: blocks b, b+8, b+16 ... share an XCD; give each XCD a contiguous run of tiles.
  const int nbn = (g.N + BN - 1) / BN, nbm = (g.M + BM - 1) / BM;
  const int nblk = nbn * nbm;
  int bid = blockIdx.x;
  {
    const int q = nblk / 8, r = nblk % 8, x = bid % 8;
    if (nblk >= 8) bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + bid / 8;
  }
  // grouped raster: runs of g.group_m tile rows are walked column by column, so the tiles an XCD's CUs hold at once
  // share A row-panels and B column-panels in its L2 (group_m = 1: plain row-major)
  int bm, bn;
  {
    const int gm = g.group_m;
    const int per_group = gm * nbn;
    const int grp = bid / per_group, first_m = grp * gm;
    const int gsz = min(nbm - first_m, gm);
    const int in = bid - grp * per_group;
    bm = first_m + in % gsz;
    bn = in / gsz;
  }
  const int m0 = bm * BM, n0 = bn * BN;

  const int nt1 = (g.K1 + BK - 1) / BK;
  // tiles made only of rows >= tail_m (the reference half of a paired pass) skip the LoRA K-tail: it is zero there
  const int nt2 = (g.a2 && m0 < g.tail_m) ? (g.K2 + BK - 1) / BK : 0;
  const int nt_all = nt1 + nt2;
  // split-K (gridDim.y > 1): this block owns K-tiles [t_beg, t_end); partials are added atomically (f32 out)
  const int per = (nt_all + gridDim.y - 1) / gridDim.y;
  const int t_beg = blockIdx.y * per;
  const int t_end = min(nt_all, t_beg + per);
  const int nt = t_end > t_beg ? t_end - t_beg : 0;
  const long a2_off = g.tail_group_n > 0 ? (long)(n0 / g.tail_group_n) * g.K2 : 0;

  // This lane's staging rows: piece i of wave w covers rows (w*A_CH + i)*8 .. +8 (B likewise).  Rows past M / N are
  // clamped onto the last valid row (their results are never stored), so the hot loop needs no row predicates and
  // every per-tile address is (per-lane constant offset) + k0: no branches, no kernel-argument reloads.
  const int prow = lane >> 3;
  const int pch = lane & 7;
  const bf16_t* zero = reinterpret_cast<const bf16_t*>(g_zero16);
  const long zb = blockIdx.z;
  const bf16_t* const a1 = g.a1 + zb * g.bat_a;
  const bf16_t* const b1 = g.b1 + zb * g.bat_b;
  void* const outp = reinterpret_cast<char*>(g.out) + zb * g.bat_o * (g.out_dtype == PSO_F32 ? 4 : 2);
  const int K1 = g.K1;
  int lcA[T::A_CH], offA[T::A_CH];  // logical chunk (source-side swizzle) and element offset of this lane's rows
  int lcB[T::B_CH], offB[T::B_CH];
  RowCoord rc[T::A_CH];
#pragma unroll
  for (int i = 0; i < T::A_CH; ++i) {
    const int R = pa(i) * 8 + prow;
    const int m = min(m0 + R, g.M - 1);
    lcA[i] = pch ^ (R & 7);
    offA[i] = CONV ? 0 : (int)((long)m * g.lda1) + lcA[i] * 8;
    if (CONV) {
      const int hw = g.conv.Ho * g.conv.Wo;
      rc[i].valid = true;
      rc[i].b = m / hw;
      const int rem = m - rc[i].b * hw;
      rc[i].oy = rem / g.conv.Wo;
      rc[i].ox = rem - rc[i].oy * g.conv.Wo;
    }
  }
#pragma unroll
  for (int i = 0; i < T::B_CH; ++i) {
    const int R = pb(i) * 8 + prow;
    const int n = min(n0 + R, g.N - 1);
    lcB[i] = pch ^ (R & 7);
    offB[i] = (int)((long)n * g.ldb1) + lcB[i] * 8;
  }
  // conv geometry in registers once
  const int cvH = g.conv.H, cvW = g.conv.W, cvS = g.conv.stride, cvP = g.conv.pad;

  auto issue_tile = [&](int tt, int buf) {
    const int t = tt + t_beg;
    bf16_t* la = stage_ptr(buf);
    bf16_t* lb = stage_ptr(buf) + BM * BK;
    if (t < nt1) {
      const int k0 = t * BK;
      const bool full = k0 + BK <= K1;  // uniform: partial last K-tile needs per-chunk predicates
      if (CONV) {
        const TapInfo ti = tap_info(g, k0);
#pragma unroll
        for (int i = 0; i < T::A_CH; ++i) {
          const int piece = pa(i);
          int iy, ix;
          bool ok;
          if (CONV == PSO_CONV_NORMAL) {
            iy = rc[i].oy * cvS + ti.kh - cvP;
            ix = rc[i].ox * cvS + ti.kw - cvP;
            ok = (unsigned)iy < (unsigned)cvH && (unsigned)ix < (unsigned)cvW;
          } else if (CONV == PSO_CONV_UP2) {
            const int uy = rc[i].oy + ti.kh - cvP, ux = rc[i].ox + ti.kw - cvP;
            ok = (unsigned)uy < (unsigned)(2 * cvH) && (unsigned)ux < (unsigned)(2 * cvW);
            iy = uy >> 1;
            ix = ux >> 1;
          } else {
            const int ty = rc[i].oy + cvP - ti.kh, tx = rc[i].ox + cvP - ti.kw;
            iy = ty >> 1;
            ix = tx >> 1;
            ok = ty >= 0 && tx >= 0 && !(ty & 1) && !(tx & 1) && iy < cvH && ix < cvW;
          }
          const bf16_t* src = ti.src + ((long)((rc[i].b * cvH + iy) * cvW + ix)) * ti.Cs + ti.c0 + lcA[i] * 8;
          __builtin_amdgcn_global_load_lds(static_cast<const void*>(ok ? src : zero), (lds_void*)(la + piece * 8 * BK), 16, 0, 0);
        }
      } else {
#pragma unroll
        for (int i = 0; i < T::A_CH; ++i) {
          const int piece = pa(i);
          const bool ok = full || k0 + lcA[i] * 8 < K1;
          __builtin_amdgcn_global_load_lds(static_cast<const void*>(ok ? a1 + offA[i] + k0 : zero), (lds_void*)(la + piece * 8 * BK), 16, 0, 0);
        }
      }
#pragma unroll
      for (int i = 0; i < T::B_CH; ++i) {
        const int piece = pb(i);
        const bool ok = full || k0 + lcB[i] * 8 < K1;
        __builtin_amdgcn_global_load_lds(static_cast<const void*>(ok ? b1 + offB[i] + k0 : zero), (lds_void*)(lb + piece * 8 * BK), 16, 0, 0);
      }
    } else {  // LoRA / second-operand K-tail (rare: one or two tiles per launch)
      const int k0 = (t - nt1) * BK;
#pragma unroll
      for (int i = 0; i < T::A_CH; ++i) {
        const int piece = pa(i);
        const int R = piece * 8 + prow;
        const int mr = m0 + R;
        const int m = min(mr, g.tail_m - 1);
        const int k = k0 + lcA[i] * 8;
        const bf16_t* src = g.a2 + a2_off + (long)m * g.lda2 + k;
        __builtin_amdgcn_global_load_lds(static_cast<const void*>((k < g.K2 && mr < g.tail_m) ? src : zero),
                                         (lds_void*)(la + piece * 8 * BK), 16, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < T::B_CH; ++i) {
        const int piece = pb(i);
        const int R = piece * 8 + prow;
        const int n = min(n0 + R, g.N - 1);
        const int k = k0 + lcB[i] * 8;
        const bf16_t* src = g.b2 + (long)n * g.ldb2 + k;
        __builtin_amdgcn_global_load_lds(static_cast<const void*>(k < g.K2 ? src : zero), (lds_void*)(lb + piece * 8 * BK), 16, 0, 0);
      }
    }
  };

  f32x4 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fk = lane >> 4;
  // Epilogue operands (bias, and the residual or the per-row-group bias) for the dense bf16/f32 store path, loaded into
  // registers while the last K-tile computes instead of one dependent load per output subtile afterwards.
  const bool epi_fast = EPI == EPI_NONE && MI * NJ <= 20 && gridDim.y == 1 && g.vec_ok && n0 + BN <= g.N && !(g.resid && g.rowbias);
  uint2 ebias[NJ], eadd[MI][NJ];
  auto epi_prefetch = [&]() {
    if (!epi_fast) return;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int n = n0 + wn * (BN / WN) + j * 16 + fk * 4;
      ebias[j] = g.bias ? *reinterpret_cast<const uint2*>(g.bias + n) : make_uint2(0u, 0u);
    }
    const bf16_t* ap = g.resid ? g.resid : g.rowbias;
    if (!ap) return;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int m = min(m0 + wm * (BM / WM) + i * 16 + fr, g.M - 1);
      const long row = g.resid ? (long)m * g.ldr : (long)(m / g.rows_per_group) * g.ld_rowbias;
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        eadd[i][j] = *reinterpret_cast<const uint2*>(ap + row + n0 + wn * (BN / WN) + j * 16 + fk * 4);
    }
  };
  if constexpr (PIPE) {
    // Register-pipelined schedule (2 LDS buffers + fragments of the next K-half in registers):
    //   iteration t:  ds_read kk=1 of tile t | MFMA kk=0 of t | lgkmcnt(0), vmcnt(0) [tile t+1 landed], s_barrier |
    //                 glds tile t+2 -> buffer of t | ds_read kk=0 of t+1 | MFMA kk=1 of t
    // so LDS reads always overlap MFMAs and the barrier is the only cross-wave sync per K-tile.  WAR: buffer t is
    // re-staged only after every wave retired its reads of it (lgkmcnt(0) before the barrier).  RAW: tile t+1 is
    // read only after every wave's glds of it retired (vmcnt(0) before the same barrier).
    static_assert(STAGES == 2, "pipelined schedule uses two LDS buffers");
    bf16x8 fa0[MI], fb0[NJ], fa1[MI], fb1[NJ];
    auto read_frags = [&](int buf, int kk, bf16x8* fa, bf16x8* fb) {
      const bf16_t* la = stage_ptr(buf);
      const bf16_t* lb = stage_ptr(buf) + BM * BK;
#pragma unroll
      for (int i = 0; i < MI; ++i)
        fa[i] = *reinterpret_cast<const bf16x8*>(la + swz(wm * (BM / WM) + i * 16 + fr, kk * 4 + fk));
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        fb[j] = *reinterpret_cast<const bf16x8*>(lb + swz(wn * (BN / WN) + j * 16 + fr, kk * 4 + fk));
    };
    auto mfma_all = [&](const bf16x8* fa, const bf16x8* fb) {
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = mfma16x16x32(fb[j], fa[i], acc[i][j]);
      __builtin_amdgcn_s_setprio(0);
    };
    if (nt > 0) issue_tile(0, 0);
    if (nt > 1) issue_tile(1, 1);
    if (nt > 1) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(PIECES) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (nt > 0) read_frags(0, 0, fa0, fb0);
    PSO_S_WAITCNT(0xC07F);  // same state on both loop-header edges (see the end of the loop body)
    for (int t = 0; t < nt; ++t) {
      const int cur = t & 1;
      read_frags(cur, 1, fa1, fb1);
      mfma_all(fa0, fb0);
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      if (t + 2 < nt) issue_tile(t + 2, cur);
      read_frags(cur ^ 1, 0, fa0, fb0);  // unconditional (past the last tile it reads a dead buffer, never used)
      // kk=1 fragments landed; the MI+NJ kk=0 reads just issued stay in flight behind these MFMAs
      static_assert(MI + NJ <= 15, "lgkmcnt field");
      PSO_S_WAITCNT(0xC07F | ((MI + NJ) << 8));
      mfma_all(fa1, fb1);
      // retire the kk=0 fragment reads HERE (behind the MFMAs) with a waitcnt the compiler can see, so the next
      // iteration's MFMAs on them do not wait for the kk=1 reads issued just before (LDS returns in order, but the
      // waitcnt pass merges the loop back-edge conservatively).  0xC07F = vmcnt(63) expcnt(7) lgkmcnt(0).
      PSO_S_WAITCNT(0xC07F);
    }
  } else {
  // prologue: K-tiles 0 .. STAGES-2 in flight; wait for tile 0
#pragma unroll
  for (int s = 0; s < STAGES - 1; ++s)
    if (s < nt) issue_tile(s, s);
  // tile 0 landed; tiles 1 .. STAGES-2 may stay in flight
  static_assert(STAGES <= 5, "vm_wait_barrier covers rings of up to 5 stages");
  vm_wait_barrier<PIECES, false>(min(STAGES - 2, nt - 1));

  int cur = 0;
  auto mfma_half = [&](const bf16_t* la, const bf16_t* lb, int kk) {
    bf16x8 af[MI], bfr[NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
      af[i] = *reinterpret_cast<const bf16x8*>(la + swz(wm * (BM / WM) + i * 16 + fr, kk * 4 + fk));
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      bfr[j] = *reinterpret_cast<const bf16x8*>(lb + swz(wn * (BN / WN) + j * 16 + fr, kk * 4 + fk));
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[i][j] = mfma16x16x32(bfr[j], af[i], acc[i][j]);
    __builtin_amdgcn_s_setprio(0);
  };
  // a LoRA K-tail of rank <= 32 fills only the first 32-deep half of its (last) K-tile, the rest being zero padding:
  // that tile is peeled off the loop and multiplies its first half only
  const bool half_last = nt > 0 && nt2 == 1 && g.K2 <= 32 && t_end == nt_all;
  const int nt_loop = nt - (half_last ? 1 : 0);
  for (int t = 0; t < nt_loop; ++t) {
    const bool ahead = t + STAGES - 1 < nt;
    if (ahead) issue_tile(t + STAGES - 1, (cur + STAGES - 1) % STAGES);
    const bf16_t* la = stage_ptr(cur);
    const bf16_t* lb = stage_ptr(cur) + BM * BK;
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) mfma_half(la, lb, kk);
    // K-tile t+1 must have landed (every wave's pieces) before anyone reads it; tiles t+2 .. stay in flight
    vm_wait_barrier<PIECES, true>(min(STAGES - 2, nt - t - 2));
    cur = (cur + 1 == STAGES) ? 0 : cur + 1;
  }
  if (half_last) {  // landed: the last loop iteration waited for it (vmcnt(0): nothing was issued beyond it)
    mfma_half(stage_ptr(cur), stage_ptr(cur) + BM * BK, 0);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
  }  // !PIPE

  // ---- epilogue: lane holds out[m][n0..n0+3] for each (i, j) ----
  if constexpr (EPI == EPI_NONE && !PIPE) {
    if (g.ws) {  // deterministic split-K: this split's partial product (every split stores, empty ones zeros)
      float* part = g.ws + (long)blockIdx.y * g.M * g.N;
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int m = m0 + wm * (BM / WM) + i * 16 + fr;
        if (m >= g.M) continue;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int n = n0 + wn * (BN / WN) + j * 16 + fk * 4;
          if (n < g.N)
            *reinterpret_cast<float4*>(part + (long)m * g.N + n) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2],
                                                                              acc[i][j][3]);
        }
      }
      return;
    }
  }
  if constexpr (EPI == EPI_GEGLU) {
    // this wave's 64 columns = one interleaved group: subtiles j = 0,1 hold h, j = 2,3 the matching gate columns.
    // h and gate are rounded to bf16 first (the unfused path stores them in bf16 before the GEGLU).
    static_assert(NJ == 4, "GEGLU epilogue needs 64-column wave tiles");
    const int ng = n0 + wn * 64;
    // the bias of this lane's 2 x 4 h / gate columns, loaded once up front (the stores below may alias it for the
    // compiler, which would otherwise reload it per row subtile behind each store)
    float bhv[2][4], bgv[2][4];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int nh = ng + jj * 16 + fk * 4;
      const uint2 bh = *reinterpret_cast<const uint2*>(g.bias + nh);
      const uint2 bg = *reinterpret_cast<const uint2*>(g.bias + nh + 32);
      bhv[jj][0] = bf2f(bh.x & 0xffff); bhv[jj][1] = bf2f(bh.x >> 16); bhv[jj][2] = bf2f(bh.y & 0xffff); bhv[jj][3] = bf2f(bh.y >> 16);
      bgv[jj][0] = bf2f(bg.x & 0xffff); bgv[jj][1] = bf2f(bg.x >> 16); bgv[jj][2] = bf2f(bg.y & 0xffff); bgv[jj][3] = bf2f(bg.y >> 16);
    }
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int m = m0 + wm * (BM / WM) + i * 16 + fr;
      if (m >= g.M) continue;
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int nh = ng + jj * 16 + fk * 4;
        float vh[4], vg[4], o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          vh[r] = bf_round(acc[i][jj][r] * g.alpha + bhv[jj][r]);
          vg[r] = bf_round(acc[i][jj + 2][r] * g.alpha + bgv[jj][r]);
          o[r] = vh[r] * gelu_erf(vg[r]);
        }
        if (g.out2 && m < g.tail_m) {  // pre-activation rows kept for the backward (policy rows of a paired pass)
          bf16_t* p = reinterpret_cast<bf16_t*>(g.out2) + (long)m * g.ldo2 + nh;
          *reinterpret_cast<uint2*>(p) = make_uint2(pack2bf(vh[0], vh[1]), pack2bf(vh[2], vh[3]));
          *reinterpret_cast<uint2*>(p + 32) = make_uint2(pack2bf(vg[0], vg[1]), pack2bf(vg[2], vg[3]));
        }
        *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(outp) + (long)m * g.ldo + ng / 2 + jj * 16 + fk * 4) =
            make_uint2(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]));
      }
    }
    return;
  }
  if constexpr (EPI == EPI_GEGLU_BWD) {
    // GEGLU backward epilogue, staged through LDS so every global access is a coalesced 16-B chunk: dout is rounded to
    // bf16 into LDS (exactly what the unfused path stores), then the workgroup walks it in 8-column chunks, reading
    // the interleaved pre-activation and writing the interleaved input gradient.
    constexpr int TP = (BM * (BN + 8) * 2 <= STAGES * (BM + BN) * BK * 2) ? BN + 8 : BN;  // tile pitch (elements)
    constexpr int NT = 64 * WM * WN;
    __syncthreads();  // every wave is done with the operand ring
    bf16_t* tl = lds_base;
    const float bscale = g.alpha;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int ml = wm * (BM / WM) + i * 16 + fr;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int nl = wn * (BN / WN) + j * 16 + fk * 4;
        float v[4] = {acc[i][j][0] * bscale, acc[i][j][1] * bscale, acc[i][j][2] * bscale, acc[i][j][3] * bscale};
        *reinterpret_cast<uint2*>(tl + ml * TP + nl) = make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
      }
    }
    __syncthreads();
    {
      // dout chunk (row ml, columns c .. c+7 of the F-wide gradient) -> interleaved positions ph .. ph+7 (gate +32)
      constexpr int CC = BN / 8;
      constexpr int ITERS = (BM * CC + NT - 1) / NT;
      // every pre-activation load of this thread in flight at once (the output stores may alias them for the
      // compiler, which would otherwise serialise one HBM round trip per chunk)
      uint4 hvv[ITERS], gvv[ITERS];
#pragma unroll
      for (int it = 0; it < ITERS; ++it) {
        const int q = threadIdx.x + it * NT;
        const int ml = q / CC, cl = (q - (q / CC) * CC) * 8;
        const int m = min(m0 + ml, g.M - 1), n = min(n0 + cl, g.N - 8);
        const int ph = (n >> 5) * 64 + (n & 31);
        if (q < BM * CC) {
          hvv[it] = *reinterpret_cast<const uint4*>(g.aux + (long)m * g.ldaux + ph);
          gvv[it] = *reinterpret_cast<const uint4*>(g.aux + (long)m * g.ldaux + ph + 32);
        }
      }
#pragma unroll
      for (int it = 0; it < ITERS; ++it) {
        const int q = threadIdx.x + it * NT;
        const int ml = q / CC, cl = (q - (q / CC) * CC) * 8;
        const int m = m0 + ml, n = n0 + cl;
        if (q >= BM * CC || m >= g.M || n >= g.N) continue;
        const int ph = (n >> 5) * 64 + (n & 31);
        const uint4 dv = *reinterpret_cast<const uint4*>(tl + ml * TP + cl);
        const uint4 hv = hvv[it], gv = gvv[it];
        const uint32_t dw[4] = {dv.x, dv.y, dv.z, dv.w}, hw[4] = {hv.x, hv.y, hv.z, hv.w}, gw[4] = {gv.x, gv.y, gv.z, gv.w};
        uint32_t oh[4], og[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d0 = bf2f(dw[e] & 0xffff), d1 = bf2f(dw[e] >> 16);
          const float h0 = bf2f(hw[e] & 0xffff), h1 = bf2f(hw[e] >> 16);
          const float g0 = bf2f(gw[e] & 0xffff), g1 = bf2f(gw[e] >> 16);
          float c0, e0, c1, e1;
          gelu_erf_parts(g0, c0, e0);
          gelu_erf_parts(g1, c1, e1);
          oh[e] = pack2bf(d0 * g0 * c0, d1 * g1 * c1);
          og[e] = pack2bf(d0 * h0 * (c0 + 0.39894228040143268f * g0 * e0), d1 * h1 * (c1 + 0.39894228040143268f * g1 * e1));
        }
        bf16_t* p = reinterpret_cast<bf16_t*>(outp) + (long)m * g.ldo + ph;
        *reinterpret_cast<uint4*>(p) = make_uint4(oh[0], oh[1], oh[2], oh[3]);
        *reinterpret_cast<uint4*>(p + 32) = make_uint4(og[0], og[1], og[2], og[3]);
      }
    }
    return;
  }
  if constexpr (EPI == EPI_NONE && !PIPE && BM * (BN + 8) * 2 <= STAGES * (BM + BN) * BK * 2) {
    if (g.stage_epi && epi_fast && g.out_dtype == PSO_ELEM && !g.accumulate && nt > 0) {
      // Staged epilogue: y = bf16(acc * alpha + bias [+ rowbias]) goes to LDS in the MFMA layout, then the workgroup
      // walks the tile in 16-B chunks: residual loaded and output stored as whole 16-B vectors (half the store
      // instructions of the 8-B per-lane layout).  The residual is added to the bf16-rounded projection, as the
      // unfused Linear + add does.
      constexpr int TP = BN + 8;
      constexpr int NT = 64 * WM * WN;
      constexpr int CC = BN / 8;
      constexpr int ITERS = (BM * CC + NT - 1) / NT;
      const bool rowb = g.rowbias != nullptr;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int n = n0 + wn * (BN / WN) + j * 16 + fk * 4;
        ebias[j] = g.bias ? *reinterpret_cast<const uint2*>(g.bias + n) : make_uint2(0u, 0u);
      }
      if (rowb) {
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          const int m = min(m0 + wm * (BM / WM) + i * 16 + fr, g.M - 1);
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            eadd[i][j] = *reinterpret_cast<const uint2*>(g.rowbias + (long)(m / g.rows_per_group) * g.ld_rowbias + n0 +
                                                         wn * (BN / WN) + j * 16 + fk * 4);
        }
      }
      __syncthreads();  // every wave is done with the operand ring
      bf16_t* tl = lds_base;
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int ml = wm * (BM / WM) + i * 16 + fr;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int nl = wn * (BN / WN) + j * 16 + fk * 4;
          float v[4] = {acc[i][j][0] * g.alpha + bf2f(ebias[j].x & 0xffff), acc[i][j][1] * g.alpha + bf2f(ebias[j].x >> 16),
                        acc[i][j][2] * g.alpha + bf2f(ebias[j].y & 0xffff), acc[i][j][3] * g.alpha + bf2f(ebias[j].y >> 16)};
          if (rowb) {
            v[0] += bf2f(eadd[i][j].x & 0xffff); v[1] += bf2f(eadd[i][j].x >> 16);
            v[2] += bf2f(eadd[i][j].y & 0xffff); v[3] += bf2f(eadd[i][j].y >> 16);
          }
          *reinterpret_cast<uint2*>(tl + ml * TP + nl) = make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
        }
      }
      // residual chunks: every load in flight at once (the accumulators are dead now)
      uint4 rr[ITERS];
      if (g.resid) {
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
          const int q = threadIdx.x + it * NT;
          const int ml = q / CC, cl = (q - (q / CC) * CC) * 8;
          const int m = min(m0 + ml, g.M - 1);
          if (q < BM * CC) rr[it] = *reinterpret_cast<const uint4*>(g.resid + (long)m * g.ldr + n0 + cl);
        }
      }
      __syncthreads();
#pragma unroll
      for (int it = 0; it < ITERS; ++it) {
        const int q = threadIdx.x + it * NT;
        const int ml = q / CC, cl = (q - (q / CC) * CC) * 8;
        const int m = m0 + ml;
        if (q >= BM * CC || m >= g.M) continue;
        uint4 y = *reinterpret_cast<const uint4*>(tl + ml * TP + cl);
        if (g.resid) {
          const uint32_t yw[4] = {y.x, y.y, y.z, y.w}, rw[4] = {rr[it].x, rr[it].y, rr[it].z, rr[it].w};
          uint32_t o[4];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            o[e] = pack2bf(bf2f(yw[e] & 0xffff) + bf2f(rw[e] & 0xffff), bf2f(yw[e] >> 16) + bf2f(rw[e] >> 16));
          y = make_uint4(o[0], o[1], o[2], o[3]);
        }
        *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(outp) + (long)m * g.ldo + n0 + cl) = y;
      }
      return;
    }
  }
  if (!PIPE && epi_fast && nt > 0) {
    epi_prefetch();  // every epilogue load in flight at once, then the arithmetic and the stores
    const bool has_add = g.resid || g.rowbias;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int m = m0 + wm * (BM / WM) + i * 16 + fr;
      if (m >= g.M) continue;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int n = n0 + wn * (BN / WN) + j * 16 + fk * 4;
        // same association as the generic path below: ((acc*alpha + bias) + rowbias | resid)
        float v[4] = {acc[i][j][0] * g.alpha + bf2f(ebias[j].x & 0xffff), acc[i][j][1] * g.alpha + bf2f(ebias[j].x >> 16),
                      acc[i][j][2] * g.alpha + bf2f(ebias[j].y & 0xffff), acc[i][j][3] * g.alpha + bf2f(ebias[j].y >> 16)};
        if (has_add) {
          v[0] += bf2f(eadd[i][j].x & 0xffff); v[1] += bf2f(eadd[i][j].x >> 16);
          v[2] += bf2f(eadd[i][j].y & 0xffff); v[3] += bf2f(eadd[i][j].y >> 16);
        }
        if (g.out_dtype == PSO_ELEM) {
          *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(outp) + (long)m * g.ldo + n) =
              make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
        } else {
          float4* o = reinterpret_cast<float4*>(reinterpret_cast<float*>(outp) + (long)m * g.ldo + n);
          if (g.accumulate) {
            const float4 old = *o;
            v[0] += old.x; v[1] += old.y; v[2] += old.z; v[3] += old.w;
          }
          *o = make_float4(v[0], v[1], v[2], v[3]);
        }
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int m = m0 + wm * (BM / WM) + i * 16 + fr;
    if (m >= g.M) continue;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int n = n0 + wn * (BN / WN) + j * 16 + fk * 4;
      if (n >= g.N) continue;
      float v[4] = {acc[i][j][0] * g.alpha, acc[i][j][1] * g.alpha, acc[i][j][2] * g.alpha,
                    acc[i][j][3] * g.alpha};
      if (gridDim.y > 1) {  // split-K partial: f32 accumulate output, no bias / residual (host-checked)
        float* o = reinterpret_cast<float*>(outp) + (long)m * g.ldo + n;
        for (int r = 0; r < 4 && n + r < g.N; ++r) atomicAdd(o + r, v[r]);
        continue;
      }
      const bool full = g.vec_ok && (n + 4 <= g.N);
      if (full) {
        if (g.bias) {
          const uint2 bv = *reinterpret_cast<const uint2*>(g.bias + n);
          v[0] += bf2f(bv.x & 0xffff); v[1] += bf2f(bv.x >> 16); v[2] += bf2f(bv.y & 0xffff); v[3] += bf2f(bv.y >> 16);
        }
        if (g.rowbias) {
          const uint2 bv = *reinterpret_cast<const uint2*>(g.rowbias + (long)(m / g.rows_per_group) * g.ld_rowbias + n);
          v[0] += bf2f(bv.x & 0xffff); v[1] += bf2f(bv.x >> 16); v[2] += bf2f(bv.y & 0xffff); v[3] += bf2f(bv.y >> 16);
        }
        if (g.resid) {
          const uint2 rv = *reinterpret_cast<const uint2*>(g.resid + (long)m * g.ldr + n);
          v[0] += bf2f(rv.x & 0xffff); v[1] += bf2f(rv.x >> 16); v[2] += bf2f(rv.y & 0xffff); v[3] += bf2f(rv.y >> 16);
        }
        if (g.out_dtype == PSO_ELEM) {
          *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(outp) + (long)m * g.ldo + n) =
              make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
        } else {
          float4* o = reinterpret_cast<float4*>(reinterpret_cast<float*>(outp) + (long)m * g.ldo + n);
          if (g.accumulate) {
            const float4 old = *o;
            v[0] += old.x; v[1] += old.y; v[2] += old.z; v[3] += old.w;
          }
          *o = make_float4(v[0], v[1], v[2], v[3]);
        }
      } else {
        for (int r = 0; r < 4 && n + r < g.N; ++r) {
          float x = v[r];
          if (g.bias) x += bf2f(g.bias[n + r]);
          if (g.rowbias) x += bf2f(g.rowbias[(long)(m / g.rows_per_group) * g.ld_rowbias + n + r]);
          if (g.resid) x += bf2f(g.resid[(long)m * g.ldr + n + r]);
          if (g.out_dtype == PSO_ELEM) {
            reinterpret_cast<bf16_t*>(outp)[(long)m * g.ldo + n + r] = f2bf(x);
          } else {
            float* o = reinterpret_cast<float*>(outp) + (long)m * g.ldo + n + r;
            *o = g.accumulate ? *o + x : x;
          }
        }
      }
    }
  }
}

template <int BM, int BN, int WM = 2, int WN = 2, int STAGES = 2, bool PIPE = false, int EPI = EPI_NONE>
static int launch(const GemmArgs& g, hipStream_t st, int ksplit = 1) {
  const int nblk = ((g.M + BM - 1) / BM) * ((g.N + BN - 1) / BN);
  dim3 grid(nblk, ksplit, g.batch > 1 ? g.batch : 1);
  const int threads = 64 * WM * WN;
  const size_t shm = (size_t)STAGES * (BM + BN) * BK * sizeof(bf16_t);
  pso_note_kernel("gemm_bf16_kernel<%d, %d, %d, %d, %d, %d, %s, %d>", BM, BN, EPI != EPI_NONE ? 0 : g.conv.mode, WM, WN,
                  STAGES, PIPE ? "true" : "false", EPI);
  static bool attr_done = false;  // >64 KiB dynamic LDS needs the attribute once per instantiation
  if constexpr (EPI != EPI_NONE) {  // fused-activation epilogues: dense operands only
    if (!attr_done) {
      (void)hipFuncSetAttribute((const void*)gemm_bf16_kernel<BM, BN, 0, WM, WN, STAGES, PIPE, EPI>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
      attr_done = true;
    }
    gemm_bf16_kernel<BM, BN, 0, WM, WN, STAGES, PIPE, EPI><<<grid, threads, shm, st>>>(g);
    return pso_check_launch("pso_gemm(geglu)");
  }
  if (!attr_done) {
    (void)hipFuncSetAttribute((const void*)gemm_bf16_kernel<BM, BN, 0, WM, WN, STAGES, PIPE, EPI>,
                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
    (void)hipFuncSetAttribute((const void*)gemm_bf16_kernel<BM, BN, PSO_CONV_NORMAL, WM, WN, STAGES, PIPE, EPI>,
                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
    (void)hipFuncSetAttribute((const void*)gemm_bf16_kernel<BM, BN, PSO_CONV_UP2, WM, WN, STAGES, PIPE, EPI>,
                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
    (void)hipFuncSetAttribute((const void*)gemm_bf16_kernel<BM, BN, PSO_CONV_T2, WM, WN, STAGES, PIPE, EPI>,
                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
    attr_done = true;
  }
  switch (g.conv.mode) {
    case PSO_CONV_NORMAL:
      gemm_bf16_kernel<BM, BN, PSO_CONV_NORMAL, WM, WN, STAGES, PIPE, EPI><<<grid, threads, shm, st>>>(g);
      break;
    case PSO_CONV_UP2: gemm_bf16_kernel<BM, BN, PSO_CONV_UP2, WM, WN, STAGES, PIPE, EPI><<<grid, threads, shm, st>>>(g); break;
    case PSO_CONV_T2: gemm_bf16_kernel<BM, BN, PSO_CONV_T2, WM, WN, STAGES, PIPE, EPI><<<grid, threads, shm, st>>>(g); break;
    default: gemm_bf16_kernel<BM, BN, 0, WM, WN, STAGES, PIPE, EPI><<<grid, threads, shm, st>>>(g);
  }
  return pso_check_launch("pso_gemm");
}

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static bool al8(const void* p) { return ((uintptr_t)p & 7) == 0; }

int pso_gemm_skinny_nt(int M, int N, int K, const void* A, long lda, const void* W, long ldw, float alpha, void* out,
                       long ldo, int out_f32, int accumulate, int groups, hipStream_t st);
int pso_gemm_tn_rank(int M, int C, const void* X, long ldx, const void* U, long ldu, int R, int group_c, float alpha,
                     float* out, long ldo, int out_jc, hipStream_t st);

static bool fits30(long rows, long ld) { return rows * ld < (1L << 30); }
int pso_conv3x3_smallc_run(int B, int H, int W, int Cin, int Cout, const void* x, const void* w, const void* bias,
                           void* out, hipStream_t st);  // conv_small.hip

// Ordered reduction of the split-K partials + the plain epilogue (4 consecutive columns per thread, N % 4 == 0):
//   y = alpha * sum_s ws[s][m][n] + bias[n] + rowbias[m / rows_per_group][n]
//   bf16 out: out = bf16(bf16(y) + resid) (the staged epilogue's rounding: the residual is added to the rounded
//             projection, as the unfused Linear + add does), f32 out: out (+)= y + resid
__global__ void gemm_splitk_reduce_kernel(GemmArgs g, int ks) {
  const long q = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const int nq = g.N / 4;
  if (q >= (long)g.M * nq) return;
  const int m = (int)(q / nq), n = (int)(q - (long)m * nq) * 4;
  const float* src = g.ws + (long)m * g.N + n;
  float4 acc = *reinterpret_cast<const float4*>(src);
  for (int s = 1; s < ks; ++s) {
    const float4 v = *reinterpret_cast<const float4*>(src + (long)s * g.M * g.N);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  float v[4] = {acc.x * g.alpha, acc.y * g.alpha, acc.z * g.alpha, acc.w * g.alpha};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (g.bias) v[r] += bf2f(g.bias[n + r]);
    if (g.rowbias) v[r] += bf2f(g.rowbias[(long)(m / g.rows_per_group) * g.ld_rowbias + n + r]);
  }
  if (g.out_dtype == PSO_ELEM) {
    if (g.resid) {
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = bf2f(f2bf(v[r])) + bf2f(g.resid[(long)m * g.ldr + n + r]);
    }
    bf16_t* o = reinterpret_cast<bf16_t*>(g.out) + (long)m * g.ldo + n;
    *reinterpret_cast<uint2*>(o) = make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
  } else {
    float* o = reinterpret_cast<float*>(g.out) + (long)m * g.ldo + n;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (g.resid) v[r] += bf2f(g.resid[(long)m * g.ldr + n + r]);
      o[r] = g.accumulate ? o[r] + v[r] : v[r];
    }
  }
}

// Benchmark knobs (gemm_plan.h GemmKnobs): mutable state in the tools build only
#ifdef PSO_BENCH_KNOBS
static GemmKnobs g_gemm_knobs = [] {
  GemmKnobs k;
  const char* e = getenv("PSO_TN128");  // benchmark knob: 0 keeps the 64 x 64 TN kernel instead of the atomic 128 x 128
  k.tn128_off = e && atoi(e) == 0;
  return k;
}();
#else
static constexpr GemmKnobs g_gemm_knobs{};
#endif
int pso_gemm_group_knob() { return g_gemm_knobs.group; }  // gemm8p.hip: a forced group is used as given

// The facts gemm_plan.h decides on.  This is the only place that looks at the pointers of a GemmArgs.
static GemmFacts gemm_facts(const GemmArgs& g, size_t ws_bytes, bool small_conv_entry) {
  const ConvGeom& cv = g.conv;
  const long hw = (long)cv.Ho * cv.Wo;
  GemmFacts f{};
  f.M = g.M; f.N = g.N; f.K1 = g.K1; f.K2 = g.a2 ? g.K2 : 0; f.has_tail = g.a2 != nullptr;
  f.tail_group_n = g.tail_group_n; f.tail_m = g.tail_m; f.batch = g.batch;
  f.out_dtype = g.out_dtype; f.accumulate = g.accumulate;
  f.has_bias = g.bias != nullptr; f.has_rowbias = g.rowbias != nullptr; f.has_resid = g.resid != nullptr;
  f.conv_mode = cv.mode; f.B = hw > 0 ? (int)(g.M / hw) : 0; f.C1 = cv.C1; f.C2 = cv.C2; f.H = cv.H; f.W = cv.W;
  f.Ho = cv.Ho; f.Wo = cv.Wo; f.ks = cv.ks; f.stride = cv.stride; f.pad = cv.pad;
  f.ab16 = al16(g.a1) && al16(g.b1);
  f.ld_ab8 = (g.lda1 % 8) == 0 && (g.ldb1 % 8) == 0;
  f.ld_ab_eq = g.lda1 == g.ldb1;
  f.out16 = al16(g.out); f.out_vec = g.out_dtype == PSO_F32 ? al16(g.out) : al8(g.out);
  f.ldo8 = (g.ldo % 8) == 0; f.ldo4 = (g.ldo % 4) == 0;
  f.resid16 = !g.resid || (al16(g.resid) && (g.ldr % 8) == 0);
  f.resid8 = !g.resid || (al8(g.resid) && (g.ldr % 4) == 0);
  f.bias8 = !g.bias || al8(g.bias);
  f.rowbias8 = !g.rowbias || al8(g.rowbias);
  f.ld_rowbias4 = !g.rowbias || (g.ld_rowbias % 4) == 0;
  f.rowgroup_hw = g.rows_per_group == hw;
  f.fits_a = fits30(g.M, g.lda1); f.fits_b = fits30(g.N, g.ldb1);
  f.fits_tail = fits30(g.tail_m, g.lda2) && fits30(g.N, g.ldb2);
  f.fits_conv = fits30((long)g.M + 2L * (cv.W + 1), cv.C1);
  f.have_ws = g.ws && al16(g.ws); f.ws_bytes = ws_bytes;
  f.small_conv_entry = small_conv_entry;
  return f;
}

// The 2-phase tile of a plan.  The product library instantiates the tiles the automatic rules choose; the forced ones
// (A/B and tests) exist in the tools build only.  A tile that is not compiled is an error, never another tile.
#define PSO_TILE(BM, BN, WM, WN, ST, PIPE, EPI) \
  if (p.epi == EPI && p.tile_is(BM, BN, WM, WN, ST, PIPE)) return launch<BM, BN, WM, WN, ST, PIPE, EPI>(g, st, ks)
static int launch_tile(const GemmPlan& p, const GemmArgs& g, hipStream_t st, int ks) {
  PSO_TILE(64, 64, 2, 2, 2, false, EPI_NONE);
  PSO_TILE(64, 128, 2, 2, 2, false, EPI_NONE);
  PSO_TILE(128, 64, 2, 2, 2, false, EPI_NONE);
  PSO_TILE(64, 160, 2, 2, 2, false, EPI_NONE);
  PSO_TILE(128, 128, 2, 4, 2, false, EPI_NONE);
  PSO_TILE(128, 160, 2, 2, 2, false, EPI_NONE);
  PSO_TILE(256, 256, 2, 4, 2, false, EPI_NONE);
  PSO_TILE(256, 256, 2, 4, 2, false, EPI_GEGLU);
  PSO_TILE(128, 160, 2, 2, 2, false, EPI_GEGLU_BWD);
  PSO_TILE(64, 64, 2, 2, 2, false, EPI_GEGLU_BWD);
#ifdef PSO_BENCH_KNOBS
#define PSO_FORCED(V, OK, BM, BN, WM, WN, ST, PIPE) PSO_TILE(BM, BN, WM, WN, ST, PIPE, EPI_NONE);
  PSO_FORCED_TILES(PSO_FORCED)
#undef PSO_FORCED
  PSO_TILE(128, 128, 2, 2, 2, false, EPI_GEGLU);
  PSO_TILE(128, 256, 2, 4, 2, false, EPI_GEGLU);
  PSO_TILE(256, 128, 4, 2, 2, false, EPI_GEGLU);
  PSO_TILE(128, 128, 2, 2, 3, false, EPI_GEGLU);
#endif
  pso_set_error("pso_gemm: tile %d x %d (%d x %d waves, %d stages%s, epilogue %d) is not compiled into this library",
                p.BM, p.BN, p.WM, p.WN, p.STAGES, p.PIPE ? ", pipelined" : "", p.epi);
  return PSO_ERR_UNSUPPORTED;
}
#undef PSO_TILE

// Launch what the plan says (g.vec_ok / stage_epi / group_m / ws are the plan's)
static int run_plan(const GemmPlan& p, GemmArgs& g, hipStream_t st) {
  g.stage_epi = p.stage_epi; g.vec_ok = p.vec_ok; g.group_m = p.group_m;
  if (p.ws_ks < 2) g.ws = nullptr;
  switch (p.form) {
    case GF_NONE: return PSO_OK;
    case GF_SKINNY:
      return pso_gemm_skinny_nt(g.M, g.N, g.K1, g.a1, g.lda1, g.b1, g.ldb1, g.alpha, g.out, g.ldo,
                                g.out_dtype == PSO_F32, g.accumulate, 1, st);
    case GF_SMALL_CONV:
      return pso_conv3x3_smallc_run(g.M / (g.conv.H * g.conv.W), g.conv.H, g.conv.W, g.conv.C1, g.N, g.a1, g.b1, g.bias,
                                    g.out, st);
    case GF_8P256: return pso_gemm8p_launch(256, p.epi, false, gemm8_args(g), st);
    case GF_8P160: return pso_gemm8p_launch(160, p.epi, false, gemm8_args(g), st);
    case GF_8P320: return pso_gemm8p_launch(320, p.epi, false, gemm8_args(g), st);
    case GF_8P320_CONV: return pso_gemm8p_launch(320, p.epi, true, gemm8_args(g), st);
    case GF_TILE: break;
    default: pso_set_error("pso_gemm: bad plan form %d", p.form); return PSO_ERR_UNSUPPORTED;
  }
  if (p.ws_ks >= 2) {  // every split stores its partial product; reduced in split order with the epilogue
    launch_tile(p, g, st, p.ws_ks);
    const long n4 = (long)g.M * (g.N / 4);
    gemm_splitk_reduce_kernel<<<(unsigned)((n4 + 255) / 256), 256, 0, st>>>(g, p.ws_ks);
    return pso_check_launch("pso_gemm_ws");
  }
  return launch_tile(p, g, st, p.atomic_ks);
}

// ws_bytes: the size of the workspace g.ws (pso_gemm_ws / pso_conv2d_ws); small_conv_entry: gemm_plan.h GemmFacts
static int run_gemm(GemmArgs& g, hipStream_t st, size_t ws_bytes = 0, bool small_conv_entry = false) {
  GemmFacts f = gemm_facts(g, ws_bytes, small_conv_entry);
  GemmPlan p = gemm_plan(f, g_gemm_knobs);
  if (p.form == GF_SMALL_CONV) {  // a failed direct convolution falls back to the GEMM forms
    if (run_plan(p, g, st) == PSO_OK) return PSO_OK;
    f.small_conv_entry = false;
    p = gemm_plan(f, g_gemm_knobs);
  }
  if (p.form != GF_NONE && g.tail_group_n > 0 && (g.tail_group_n % 64) != 0) {
    pso_set_error("pso_gemm: tail_group_n must be a multiple of 64");
    return PSO_ERR_ARG;
  }
  return run_plan(p, g, st);
}

// =====================================================================================================================
// TN GEMM: out[I][J] (+)= alpha * sum_m A[m][I] * B[m][J]   (both operands "token-major": the reduction index is the
// row index).  This is the shape of every LoRA weight gradient (dA = v^T x, dB = s dy^T u, reduction over the
// B*S tokens); it replaces two explicit transposes per product.  Tiles of 64 (m) rows x 64 columns are staged
// row-major in LDS with the chunk ^ (2*((row>>1)&3)) swizzle and read as MFMA fragments with ds_read_b64_tr_b16
// (lane i of a 16-lane group receives column i of 4 consecutive rows = 4 consecutive k of one output row).
// Split-K over gridDim.y with f32 atomics in the epilogue (output is always an f32 accumulator).
// =====================================================================================================================
typedef __attribute__((address_space(3))) s16x4 lds_s16x4_g;
typedef __attribute__((address_space(3))) void tnr_lds_void_g;
__device__ __forceinline__ int swz_tr64(int r, int c) { return r * 64 + ((c ^ (((r >> 1) & 3) << 1)) << 3); }

__device__ __forceinline__ s16x4 tr_read64(const bf16_t* img, int r0, int col0, int lane) {
  const int li = lane & 15;
  const int q = li >> 2, p = li & 3;
  const int col = col0 + 4 * p;
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_g*)(img + swz_tr64(r0 + q, col >> 3) + (col & 7)));
}

__global__ __launch_bounds__(256, 2) void gemm_tn_kernel(int M, int I, int J, const bf16_t* __restrict__ A, long lda,
                                                         const bf16_t* __restrict__ B, long ldb, float alpha,
                                                         float* __restrict__ out, long ldo,
                                                         float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) bf16_t sA[2][64 * 64];
  __shared__ __attribute__((aligned(16))) bf16_t sB[2][64 * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1;
  const int nbj = (J + 63) / 64;
  const int bi = blockIdx.x / nbj, bj = blockIdx.x - bi * nbj;
  const int i0 = bi * 64, j0 = bj * 64;
  const int nkt = (M + 63) / 64;
  const int per = (nkt + gridDim.y - 1) / gridDim.y;
  const int t_beg = blockIdx.y * per, t_end = min(nkt, t_beg + per);
  uint4 ra[2], rb[2];
  auto load = [&](int t) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int q = tid + 256 * h;
      const int row = q >> 3, ch = q & 7;
      const int m = t * 64 + row;
      const int ci = i0 + ch * 8, cj = j0 + ch * 8;
      ra[h] = (m < M && ci < I) ? *reinterpret_cast<const uint4*>(A + (long)m * lda + ci) : make_uint4(0, 0, 0, 0);
      rb[h] = (m < M && cj < J) ? *reinterpret_cast<const uint4*>(B + (long)m * ldb + cj) : make_uint4(0, 0, 0, 0);
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int q = tid + 256 * h;
      const int row = q >> 3, ch = q & 7;
      *reinterpret_cast<uint4*>(sA[buf] + swz_tr64(row, ch)) = ra[h];
      *reinterpret_cast<uint4*>(sB[buf] + swz_tr64(row, ch)) = rb[h];
    }
  };
  f32x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int g = lane >> 4, c = lane & 15;
  if (t_beg < t_end) {
    load(t_beg);
    store(0);
  }
  __syncthreads();
  for (int t = t_beg; t < t_end; ++t) {
    const int cur = (t - t_beg) & 1;
    if (t + 1 < t_end) load(t + 1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[2], bfr[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int col = wi * 32 + a * 16;
        typedef __attribute__((ext_vector_type(8))) short s16x8;
        const s16x4 x0 = tr_read64(sA[cur], ks * 32 + 8 * g, col, lane);
        const s16x4 x1 = tr_read64(sA[cur], ks * 32 + 8 * g + 4, col, lane);
        s16x8 v = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
        af[a] = __builtin_bit_cast(bf16x8, v);
      }
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int col = wj * 32 + b * 16;
        typedef __attribute__((ext_vector_type(8))) short s16x8;
        const s16x4 y0 = tr_read64(sB[cur], ks * 32 + 8 * g, col, lane);
        const s16x4 y1 = tr_read64(sB[cur], ks * 32 + 8 * g + 4, col, lane);
        s16x8 v = {y0[0], y0[1], y0[2], y0[3], y1[0], y1[1], y1[2], y1[3]};
        bfr[b] = __builtin_bit_cast(bf16x8, v);
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = mfma16x16x32(bfr[b], af[a], acc[a][b]);
    }
    if (t + 1 < t_end) store(cur ^ 1);
    __syncthreads();
  }
  // lane holds out[i = i0 + wi*32 + a*16 + c][j = j0 + wj*32 + b*16 + 4g + r]
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int i = i0 + wi * 32 + a * 16 + c;
    if (i >= I) continue;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int j = j0 + wj * 32 + b * 16 + 4 * g;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (j + r < J) {
          float* o = out + (long)i * ldo + j + r;
          if (part) part[((long)blockIdx.y * I + i) * J + j + r] = acc[a][b][r] * alpha;  // ordered-reduction slice
          else if (gridDim.y > 1) atomicAdd(o, acc[a][b][r] * alpha);
          else *o += acc[a][b][r] * alpha;
        }
    }
  }
}

// 128 x 128 TN tile for the full-weight gradients (C3 / C4: dW = X^T dY over the B*H*W tokens, I, J >= 128):
// 4 waves of 64 x 64 (4 x 4 MFMA tiles, every operand fragment feeds four MFMAs), 64-token K-steps staged by
// buffer_load ... lds (each wave one 64 x 64 image: A cols i0.. / i0+64.., B cols j0.. / j0+64..; source-side
// swizzle for the transposed reads; rows past M read as zeros) through a 2-stage ring, fragments by inline-asm
// ds_read_b64_tr_b16 (the builtin makes hipcc drain the LDS-DMA ring).  Split-K over gridDim.y with f32 atomics.
__device__ __forceinline__ s16x4 tn_tr_asm(unsigned img_base, int r0, int col0, int lane) {
  const int li = lane & 15;
  const int q = li >> 2, p = li & 3;
  const int col = col0 + 4 * p;
  const unsigned addr = img_base + 2u * (unsigned)(swz_tr64(r0 + q, col >> 3) + (col & 7));
  s16x4 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(addr));
  return v;
}

__global__ __launch_bounds__(256, 2) void gemm_tn128_kernel(int M, int I, int J, const bf16_t* __restrict__ A,
                                                            long lda, const bf16_t* __restrict__ B, long ldb,
                                                            float alpha, float* __restrict__ out, long ldo,
                                                            int steps, float* __restrict__ part, int geglu_f = 0) {
  __shared__ __attribute__((aligned(16))) bf16_t sT[2][4][64 * 64];  // [stage][A0 A1 B0 B1], 64 KB
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wi = wave >> 1, wj = wave & 1;
  const int g = lane >> 4, c = lane & 15;
  const int nbj = (J + 127) / 128;
  const int bi = blockIdx.x / nbj, bj = blockIdx.x - bi * nbj;
  const int i0 = bi * 128, j0 = bj * 128;
  const int nkt = (M + 63) / 64;
  const int t_beg = blockIdx.y * steps, t_end = min(nkt, t_beg + steps);
  // wave w stages image w: A (w < 2) or B, 64 columns from col0, all 8 pieces of 8 rows x 128 B
  const bool isA = wave < 2;
  const long ld = isA ? lda : ldb;
  const int col0 = (isA ? i0 : j0) + (wave & 1) * 64;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(isA ? A : B), (short)0, (int)(((long)(M - 1) * ld + (isA ? I : J)) * 2), 0x00020000);
  const int prow = lane >> 3, pch = lane & 7;
  const int sc = pch ^ (((prow >> 1) & 3) << 1);  // source chunk landing at LDS chunk pch (swz_tr64)
  // columns past I / J are clamped to the last 8 (their products land in unstored outputs)
  const int cw = min(col0 + sc * 8, (isA ? I : J) - 8);
  const unsigned voff = (unsigned)((long)prow * ld + cw) * 2u;
  const int kstep = (int)(64 * ld * 2);
  auto issue = [&](int t, int stg) {
#pragma unroll
    for (int p = 0; p < 8; ++p)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (tnr_lds_void_g*)(sT[stg][wave] + p * 8 * 64), 16,
                                               voff + (unsigned)(p * 8 * ld * 2), t * kstep, 0, 0);
  };
  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  const unsigned lbase = (unsigned)(uintptr_t)(const tnr_lds_void_g*)&sT[0][0][0];
  if (t_beg < t_end) issue(t_beg, 0);
  asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
  for (int t = t_beg; t < t_end; ++t) {
    const int cur = (t - t_beg) & 1;
    if (t + 1 < t_end) issue(t + 1, cur ^ 1);
    const unsigned ia = lbase + (unsigned)((cur * 4 + wi) * 64 * 64 * 2);
    const unsigned ib = lbase + (unsigned)((cur * 4 + 2 + wj) * 64 * 64 * 2);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      s16x4 ra[8], rb[8];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        ra[2 * a] = tn_tr_asm(ia, ks * 32 + 8 * g, a * 16, lane);
        ra[2 * a + 1] = tn_tr_asm(ia, ks * 32 + 8 * g + 4, a * 16, lane);
        rb[2 * a] = tn_tr_asm(ib, ks * 32 + 8 * g, a * 16, lane);
        rb[2 * a + 1] = tn_tr_asm(ib, ks * 32 + 8 * g + 4, a * 16, lane);
      }
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(ra[0]), "+v"(ra[1]), "+v"(ra[2]), "+v"(ra[3]), "+v"(ra[4]), "+v"(ra[5]), "+v"(ra[6]),
                     "+v"(ra[7]), "+v"(rb[0]), "+v"(rb[1]), "+v"(rb[2]), "+v"(rb[3]), "+v"(rb[4]), "+v"(rb[5]),
                     "+v"(rb[6]), "+v"(rb[7]));
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        typedef __attribute__((ext_vector_type(8))) short s16x8;
        s16x8 va = {ra[2 * a][0], ra[2 * a][1], ra[2 * a][2], ra[2 * a][3],
                    ra[2 * a + 1][0], ra[2 * a + 1][1], ra[2 * a + 1][2], ra[2 * a + 1][3]};
        s16x8 vb = {rb[2 * a][0], rb[2 * a][1], rb[2 * a][2], rb[2 * a][3],
                    rb[2 * a + 1][0], rb[2 * a + 1][1], rb[2 * a + 1][2], rb[2 * a + 1][3]};
        af[a] = __builtin_bit_cast(bf16x8, va);
        bfr[a] = __builtin_bit_cast(bf16x8, vb);
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = mfma16x16x32(bfr[b], af[a], acc[a][b]);
      __builtin_amdgcn_s_setprio(0);
    }
    // the next stage landed (every wave's pieces), and every wave's reads of this stage retired before it is restaged
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
  // lane holds out[i = i0 + wi*64 + a*16 + c][j = j0 + wj*64 + b*16 + 4g + r]
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = i0 + wi * 64 + a * 16 + c;
    if (i >= I) continue;
    // geglu_f > 0: A's columns are the GEGLU interleave (per 32 outputs [h 32 | gate 32]); row i of the product goes
    // to row (i / 64) * 32 + i % 32 of the natural [h | gate] order, plus geglu_f for the gate half
    const int io = geglu_f > 0 ? ((i >> 6) << 5) + (i & 31) + ((i & 32) ? geglu_f : 0) : i;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = j0 + wj * 64 + b * 16 + 4 * g;
      if (j >= J) continue;  // J % 8 == 0: a lane's 4 columns are all in or all out
      float* o = out + (long)io * ldo + j;
      if (part) {  // this slice's partial product, stored (added into out by tn_reduce_slices_kernel)
        *reinterpret_cast<float4*>(part + ((long)blockIdx.y * I + i) * J + j) =
            make_float4(acc[a][b][0] * alpha, acc[a][b][1] * alpha, acc[a][b][2] * alpha, acc[a][b][3] * alpha);
      } else if (gridDim.y > 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) atomicAdd(o + r, acc[a][b][r] * alpha);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] += acc[a][b][r] * alpha;
      }
    }
  }
}

// out[i][j] += sum over the ks slices of part[s][i][j], in slice order (4 consecutive j per thread)
__global__ void tn_reduce_slices_kernel(int I, int J, int ks, const float* __restrict__ part, float* __restrict__ out,
                                        long ldo) {
  const long q = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const long n4 = (long)I * J / 4;
  if (q >= n4) return;
  const long e = q * 4;
  const int i = (int)(e / J), j = (int)(e - (long)i * J);
  float4 sacc = *reinterpret_cast<const float4*>(part + e);
  for (int sl = 1; sl < ks; ++sl) {
    const float4 v = *reinterpret_cast<const float4*>(part + (long)sl * I * J + e);
    sacc.x += v.x; sacc.y += v.y; sacc.z += v.z; sacc.w += v.w;
  }
  float* o = out + (long)i * ldo + j;
  o[0] += sacc.x; o[1] += sacc.y; o[2] += sacc.z; o[3] += sacc.w;
}

// 256 x 256 TN tile for the large full-weight gradients: 8 waves of 64 x 128 (4 x 8 MFMA tiles; each A fragment
// feeds 8 MFMAs, each B fragment 4), the same per-wave 64 x 64 images and transposed reads as gemm_tn128_kernel.  A
// 128 x 128 tile moves 32 KB of operands per 2.1 MFLOP (one 64-token step) -- ~38 TB/s of L2 reads at the MFMA peak
// over 256 CUs, more than the L2s deliver; the 256 x 256 tile halves the bytes per flop.  One workgroup per CU
// (128 KB LDS: 2 stages x 8 images).  part != nullptr: this slice's partial product into the workspace (ordered
// reduction by tn_reduce_slices_kernel); else out += directly (the caller launches one slice).
__global__ __launch_bounds__(512, 1) void gemm_tn256_kernel(int M, int I, int J, const bf16_t* __restrict__ A,
                                                            long lda, const bf16_t* __restrict__ B, long ldb,
                                                            float alpha, float* __restrict__ out, long ldo,
                                                            int steps, float* __restrict__ part, int geglu_f) {
  extern __shared__ __attribute__((aligned(16))) bf16_t t256s[];  // [stage][A0 A1 A2 A3 B0 B1 B2 B3][64 x 64]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wi = wave >> 1, wj = wave & 1;
  const int g = lane >> 4, c = lane & 15;
  const int nbj = (J + 255) / 256;
  const int bi = blockIdx.x / nbj, bj = blockIdx.x - bi * nbj;
  const int i0 = bi * 256, j0 = bj * 256;
  const int nkt = (M + 63) / 64;
  const int t_beg = blockIdx.y * steps, t_end = min(nkt, t_beg + steps);
  // wave w stages image w: A columns i0 + 64 w (w < 4) or B columns j0 + 64 (w - 4), 8 pieces of 8 rows x 128 B
  const bool isA = wave < 4;
  const long ld = isA ? lda : ldb;
  const int col0 = (isA ? i0 : j0) + (wave & 3) * 64;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(isA ? A : B), (short)0, (int)(((long)(M - 1) * ld + (isA ? I : J)) * 2), 0x00020000);
  const int prow = lane >> 3, pch = lane & 7;
  const int sc = pch ^ (((prow >> 1) & 3) << 1);
  const int cw = min(col0 + sc * 8, (isA ? I : J) - 8);
  const unsigned voff = (unsigned)((long)prow * ld + cw) * 2u;
  const int kstep = (int)(64 * ld * 2);
  auto issue = [&](int t, int stg) {
#pragma unroll
    for (int p = 0; p < 8; ++p)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (tnr_lds_void_g*)(t256s + (stg * 8 + wave) * 4096 + p * 8 * 64), 16,
                                               voff + (unsigned)(p * 8 * ld * 2), t * kstep, 0, 0);
  };
  f32x4 acc[4][8];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  const unsigned lbase = (unsigned)(uintptr_t)(const tnr_lds_void_g*)t256s;
  if (t_beg < t_end) issue(t_beg, 0);
  asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
  for (int t = t_beg; t < t_end; ++t) {
    const int cur = (t - t_beg) & 1;
    if (t + 1 < t_end) issue(t + 1, cur ^ 1);
    const unsigned ia = lbase + (unsigned)((cur * 8 + wi) * 4096 * 2);
    const unsigned ib = lbase + (unsigned)((cur * 8 + 4 + 2 * wj) * 4096 * 2);  // images 4 + 2 wj, 5 + 2 wj
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      s16x4 ra[8], rb[16];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        ra[2 * a] = tn_tr_asm(ia, ks * 32 + 8 * g, a * 16, lane);
        ra[2 * a + 1] = tn_tr_asm(ia, ks * 32 + 8 * g + 4, a * 16, lane);
      }
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const unsigned im = ib + (unsigned)((b >> 2) * 4096 * 2);
        rb[2 * b] = tn_tr_asm(im, ks * 32 + 8 * g, (b & 3) * 16, lane);
        rb[2 * b + 1] = tn_tr_asm(im, ks * 32 + 8 * g + 4, (b & 3) * 16, lane);
      }
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(ra[0]), "+v"(ra[1]), "+v"(ra[2]), "+v"(ra[3]), "+v"(ra[4]), "+v"(ra[5]), "+v"(ra[6]),
                     "+v"(ra[7]), "+v"(rb[0]), "+v"(rb[1]), "+v"(rb[2]), "+v"(rb[3]));
      asm volatile(""
                   : "+v"(rb[4]), "+v"(rb[5]), "+v"(rb[6]), "+v"(rb[7]), "+v"(rb[8]), "+v"(rb[9]), "+v"(rb[10]),
                     "+v"(rb[11]), "+v"(rb[12]), "+v"(rb[13]), "+v"(rb[14]), "+v"(rb[15]));
      typedef __attribute__((ext_vector_type(8))) short s16x8;
      bf16x8 af[4], bfr[8];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        s16x8 va = {ra[2 * a][0], ra[2 * a][1], ra[2 * a][2], ra[2 * a][3],
                    ra[2 * a + 1][0], ra[2 * a + 1][1], ra[2 * a + 1][2], ra[2 * a + 1][3]};
        af[a] = __builtin_bit_cast(bf16x8, va);
      }
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        s16x8 vb = {rb[2 * b][0], rb[2 * b][1], rb[2 * b][2], rb[2 * b][3],
                    rb[2 * b + 1][0], rb[2 * b + 1][1], rb[2 * b + 1][2], rb[2 * b + 1][3]};
        bfr[b] = __builtin_bit_cast(bf16x8, vb);
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = mfma16x16x32(bfr[b], af[a], acc[a][b]);
      __builtin_amdgcn_s_setprio(0);
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
  // lane holds out[i = i0 + wi*64 + a*16 + c][j = j0 + wj*128 + b*16 + 4g + r]
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = i0 + wi * 64 + a * 16 + c;
    if (i >= I) continue;
    const int io = geglu_f > 0 ? ((i >> 6) << 5) + (i & 31) + ((i & 32) ? geglu_f : 0) : i;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const int j = j0 + wj * 128 + b * 16 + 4 * g;
      if (j >= J) continue;
      if (part) {
        *reinterpret_cast<float4*>(part + ((long)blockIdx.y * I + i) * J + j) =
            make_float4(acc[a][b][0] * alpha, acc[a][b][1] * alpha, acc[a][b][2] * alpha, acc[a][b][3] * alpha);
      } else {
        float* o = out + (long)io * ldo + j;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] += acc[a][b][r] * alpha;
      }
    }
  }
}


static void tn256_launch(int M, int I, int J, const void* A, long lda, const void* B, long ldb, float alpha, float* out,
                         long ldo, int ks, float* part, int geglu_f, hipStream_t st) {
  static bool attr = [] {
    (void)hipFuncSetAttribute((const void*)gemm_tn256_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
    return true;
  }();
  (void)attr;
  const int nkt = (M + 63) / 64;
  const int steps = (nkt + ks - 1) / ks;
  pso_note_kernel("gemm_tn256_kernel");
  gemm_tn256_kernel<<<dim3((I / 256) * (J / 256), ks), 512, 131072, st>>>(M, I, J, (const bf16_t*)A, lda,
                                                                          (const bf16_t*)B, ldb, alpha, out, ldo,
                                                                          steps, part, geglu_f);
}

// the workspace a TN plan needs (gemm_plan.h tn_plan with have_ws; 0: none)
static size_t tn_plan_ws_bytes(const TnPlan& p, int M, int I, int J) {
  if (!p.ws) return 0;
  if (p.kind != TNP_RANK) return (size_t)p.ks * I * J * sizeof(float);
  PsoTnRankProblem q{};
  q.x = (const void*)16; q.u = (const void*)16; q.out = (float*)16; q.ldx = 8; q.ldu = 8;
  q.ldo = p.swap ? I : J; q.M = M; q.C = p.swap ? J : I; q.group_c = 0; q.alpha = 1.f;
  return pso_gemm_tn_rank_batch_ws_bytes(p.rank, p.swap ? 1 : 0, 1, &q);
}

extern "C" {

size_t pso_gemm_tn_ws_bytes(int M, int I, int J) {
  if (M <= 0) return 0;
  GemmKnobs k = g_gemm_knobs;
  k.tn_split = 0;  // the size does not follow the split knob; pso_gemm_tn_ws leaves the workspace unused under it
  return tn_plan_ws_bytes(tn_plan(M, I, J, I, J, 0, true, k), M, I, J);
}

}  // extern "C"

// the tile kernels of a TN plan: part = the workspace of the plan's slices, or null (out += directly / f32 atomics)
static void tn_launch_tiles(const TnPlan& p, int M, int I, int J, const void* A, long lda, const void* B, long ldb,
                            float alpha, float* out, long ldo, float* part, hipStream_t st) {
  if (p.kind == TNP_256) {
    tn256_launch(M, I, J, A, lda, B, ldb, alpha, out, ldo, p.ks, part, 0, st);
  } else if (p.kind == TNP_128) {
    const int t128 = ((I + 127) / 128) * ((J + 127) / 128);
    pso_note_kernel("gemm_tn128_kernel");
    gemm_tn128_kernel<<<dim3(t128, p.ks), 256, 0, st>>>(M, I, J, (const bf16_t*)A, lda, (const bf16_t*)B, ldb, alpha,
                                                        out, ldo, p.steps, part);
  } else {
    const int tiles = ((I + 63) / 64) * ((J + 63) / 64);
    pso_note_kernel("gemm_tn_kernel");
    gemm_tn_kernel<<<dim3(tiles, p.ks), 256, 0, st>>>(M, I, J, (const bf16_t*)A, lda, (const bf16_t*)B, ldb, alpha,
                                                      out, ldo, part);
  }
}

// Argument checks and GemmArgs of pso_gemm / pso_gemm_ws (who = the entry's name in the messages)
static int gemm_entry_args(const char* who, GemmArgs& g, int M, int N, const void* a1, long lda1, int K1,
                           const void* b1, long ldb1, const void* a2, long lda2, int K2, const void* b2, long ldb2,
                           float alpha, const void* bias, const void* rowbias, long ld_rowbias, int rows_per_group,
                           const void* resid, long ldr, void* out, long ldo, int out_dtype, int accumulate,
                           int tail_group_n, int tail_rows) {
  PSO_ARG_CHECK(M >= 0 && N >= 0 && K1 >= 0 && (K1 % 8) == 0, "%s: need K1 %% 8 == 0 (K1=%d)", who, K1);
  PSO_ARG_CHECK(a1 && b1 && out, "%s: null operand", who);
  PSO_ARG_CHECK(al16(a1) && al16(b1) && (lda1 % 8) == 0 && (ldb1 % 8) == 0, "%s: A1/B1 must be 16-B aligned rows", who);
  PSO_ARG_CHECK(!a2 || (b2 && (K2 % 8) == 0 && al16(a2) && al16(b2) && (lda2 % 8) == 0 && (ldb2 % 8) == 0),
                "%s: bad second operand", who);
  PSO_DTYPE_CHECK(out_dtype, who);
  PSO_ARG_CHECK((long)M * lda1 < 0x7fffffffL && (long)N * ldb1 < 0x7fffffffL,
                "%s: operand spans more than 2^31 elements", who);
  PSO_ARG_CHECK(!accumulate || out_dtype == PSO_F32, "%s: accumulate needs f32 output", who);
  PSO_ARG_CHECK(!rowbias || rows_per_group > 0, "%s: rowbias needs rows_per_group > 0", who);
  g.a1 = (const bf16_t*)a1; g.lda1 = lda1; g.K1 = K1;
  g.b1 = (const bf16_t*)b1; g.ldb1 = ldb1;
  g.a2 = (const bf16_t*)a2; g.lda2 = lda2; g.K2 = a2 ? K2 : 0;
  g.b2 = (const bf16_t*)b2; g.ldb2 = ldb2;
  g.tail_group_n = a2 ? tail_group_n : 0;
  g.tail_m = (tail_rows > 0 && tail_rows < M) ? tail_rows : M;
  g.M = M; g.N = N;
  g.alpha = alpha;
  g.bias = (const bf16_t*)bias;
  g.rowbias = (const bf16_t*)rowbias; g.ld_rowbias = ld_rowbias; g.rows_per_group = rows_per_group > 0 ? rows_per_group : 1;
  g.resid = (const bf16_t*)resid; g.ldr = ldr;
  g.out = out; g.ldo = ldo; g.out_dtype = out_dtype; g.accumulate = accumulate;
  return PSO_OK;
}

// Argument checks and GemmArgs of pso_conv2d / pso_conv2d_ws
static int conv_entry_args(const char* who, GemmArgs& g, int mode, int B, const void* src1, int C1, const void* src2,
                           int C2, int H, int W, int Ho, int Wo, int ks, int stride, int pad, const void* weight,
                           int Cout, const void* a2, long lda2, int K2, const void* b2, long ldb2, float alpha,
                           const void* bias, const void* rowbias, long ld_rowbias, const void* resid, long ldr,
                           void* out, long ldo, int out_dtype, int accumulate) {
  PSO_ARG_CHECK(mode == PSO_CONV_NORMAL || mode == PSO_CONV_UP2 || mode == PSO_CONV_T2, "%s: bad mode", who);
  PSO_ARG_CHECK(src1 && weight && out, "%s: null operand", who);
  PSO_ARG_CHECK((C1 % 64) == 0 && (C2 % 64) == 0 && (C2 == 0 || src2),
                "%s: channel sources must be multiples of 64 (C1=%d C2=%d); use im2col for small C", who, C1, C2);
  PSO_ARG_CHECK(al16(src1) && (!src2 || al16(src2)) && al16(weight), "%s: alignment", who);
  PSO_ARG_CHECK(ks == 1 || ks == 3, "%s: ks must be 1 or 3", who);
  PSO_ARG_CHECK(mode != PSO_CONV_UP2 || (Ho == 2 * H && Wo == 2 * W && stride == 1), "%s: UP2 geometry", who);
  PSO_ARG_CHECK(!a2 || ((K2 % 8) == 0 && b2 && al16(a2) && al16(b2)), "%s: bad second operand", who);
  PSO_DTYPE_CHECK(out_dtype, who);
  PSO_ARG_CHECK(!accumulate || out_dtype == PSO_F32, "%s: accumulate needs f32 output", who);
  const int Ct = C1 + C2;
  g.a1 = (const bf16_t*)src1; g.lda1 = 0; g.K1 = ks * ks * Ct;
  g.b1 = (const bf16_t*)weight; g.ldb1 = g.K1;
  g.a2 = (const bf16_t*)a2; g.lda2 = lda2; g.K2 = a2 ? K2 : 0;
  g.b2 = (const bf16_t*)b2; g.ldb2 = ldb2;
  g.M = B * Ho * Wo; g.N = Cout;
  g.tail_m = g.M;
  g.conv.mode = mode; g.conv.src2 = (const bf16_t*)src2; g.conv.C1 = C1; g.conv.C2 = C2;
  g.conv.H = H; g.conv.W = W; g.conv.Ho = Ho; g.conv.Wo = Wo; g.conv.ks = ks; g.conv.stride = stride; g.conv.pad = pad;
  g.alpha = alpha;
  g.bias = (const bf16_t*)bias;
  g.rowbias = (const bf16_t*)rowbias; g.ld_rowbias = ld_rowbias; g.rows_per_group = Ho * Wo;
  g.resid = (const bf16_t*)resid; g.ldr = ldr;
  g.out = out; g.ldo = ldo; g.out_dtype = out_dtype; g.accumulate = accumulate;
  return PSO_OK;
}

// GemmArgs of pso_gemm_batched (dense, no epilogue operands)
static GemmArgs batched_args(int batch, int M, int N, int K, const void* a, long lda, long stride_a, const void* b,
                             long ldb, long stride_b, float alpha, void* out, long ldo, long stride_o, int out_dtype) {
  GemmArgs g{};
  g.a1 = (const bf16_t*)a; g.lda1 = lda; g.K1 = K;
  g.b1 = (const bf16_t*)b; g.ldb1 = ldb;
  g.M = M; g.N = N; g.tail_m = M;
  g.alpha = alpha; g.rows_per_group = 1;
  g.out = out; g.ldo = ldo; g.out_dtype = out_dtype;
  g.bat_a = stride_a; g.bat_b = stride_b; g.bat_o = stride_o; g.batch = batch;
  return g;
}

extern "C" {

int pso_gemm_tn_ws(int M, int I, int J, const void* A, long lda, const void* B, long ldb, float alpha, float* out,
                   long ldo, void* ws, size_t ws_bytes, void* stream) {
  PSO_ARG_CHECK(M >= 0 && I > 0 && J > 0 && A && B && out, "pso_gemm_tn_ws: bad args");
  PSO_ARG_CHECK(((uintptr_t)A & 15) == 0 && ((uintptr_t)B & 15) == 0 && (lda % 8) == 0 && (ldb % 8) == 0 &&
                    (I % 8) == 0 && (J % 8) == 0,
                "pso_gemm_tn_ws: operands need 16-B aligned rows and I, J multiples of 8");
  if (M == 0) return PSO_OK;
  const hipStream_t st = (hipStream_t)stream;
  const TnPlan p = tn_plan(M, I, J, lda, ldb, 0, ws && al16(ws), g_gemm_knobs);
  const size_t need = tn_plan_ws_bytes(p, M, I, J);
  // without a workspace that holds every slice: the forms of pso_gemm_tn
  if (!need || ws_bytes < need) return pso_gemm_tn_grouped(M, I, J, A, lda, B, ldb, alpha, out, ldo, 0, stream);
  if (p.kind == TNP_RANK) {
    PsoTnRankProblem q{};
    q.x = p.swap ? B : A; q.ldx = p.swap ? ldb : lda;
    q.u = p.swap ? A : B; q.ldu = p.swap ? lda : ldb;
    q.out = out; q.ldo = ldo; q.M = M; q.C = p.swap ? J : I; q.group_c = 0; q.alpha = alpha;
    return pso_gemm_tn_rank_batch_ws(p.rank, p.swap ? 1 : 0, 1, &q, ws, ws_bytes, stream);
  }
  tn_launch_tiles(p, M, I, J, A, lda, B, ldb, alpha, out, ldo, (float*)ws, st);
  const long n4 = (long)I * J / 4;
  tn_reduce_slices_kernel<<<(unsigned)((n4 + 255) / 256), 256, 0, st>>>(I, J, p.ks, (const float*)ws, out, ldo);
  return pso_check_launch("pso_gemm_tn_ws");
}

int pso_gemm(int M, int N, const void* a1, long lda1, int K1, const void* b1, long ldb1, const void* a2, long lda2,
             int K2, const void* b2, long ldb2, float alpha, const void* bias, const void* rowbias, long ld_rowbias,
             int rows_per_group, const void* resid, long ldr, void* out, long ldo, int out_dtype, int accumulate,
             int tail_group_n, int tail_rows, void* stream) {
  GemmArgs g{};
  const int rc = gemm_entry_args("pso_gemm", g, M, N, a1, lda1, K1, b1, ldb1, a2, lda2, K2, b2, ldb2, alpha, bias,
                                 rowbias, ld_rowbias, rows_per_group, resid, ldr, out, ldo, out_dtype, accumulate,
                                 tail_group_n, tail_rows);
  return rc != PSO_OK ? rc : run_gemm(g, (hipStream_t)stream);
}

size_t pso_gemm_ws_bytes(int M, int N, int K1, int K2) {
  const SplitPlan sp = gemm_split_plan(M, N, K1, K2, K2 > 0, g_gemm_knobs);
  return sp.ks >= 2 ? (size_t)sp.ks * M * N * sizeof(float) : 0;
}

// the workspace form applies when the plan splits and the caller's workspace holds every split; else pso_gemm
int pso_gemm_ws(int M, int N, const void* a1, long lda1, int K1, const void* b1, long ldb1, const void* a2, long lda2,
                int K2, const void* b2, long ldb2, float alpha, const void* bias, const void* rowbias, long ld_rowbias,
                int rows_per_group, const void* resid, long ldr, void* out, long ldo, int out_dtype, int accumulate,
                int tail_group_n, int tail_rows, void* ws, size_t ws_bytes, void* stream) {
  GemmArgs g{};
  const int rc = gemm_entry_args("pso_gemm_ws", g, M, N, a1, lda1, K1, b1, ldb1, a2, lda2, K2, b2, ldb2, alpha, bias,
                                 rowbias, ld_rowbias, rows_per_group, resid, ldr, out, ldo, out_dtype, accumulate,
                                 tail_group_n, tail_rows);
  g.ws = (float*)ws;
  return rc != PSO_OK ? rc : run_gemm(g, (hipStream_t)stream, ws_bytes);
}

int pso_gemm_batched(int batch, int M, int N, int K, const void* a, long lda, long stride_a, const void* b, long ldb,
                     long stride_b, float alpha, void* out, long ldo, long stride_o, int out_dtype, void* stream) {
  PSO_ARG_CHECK(batch >= 1 && M >= 0 && N >= 0 && K >= 0 && (K % 8) == 0, "pso_gemm_batched: bad shape (K %% 8 == 0)");
  PSO_ARG_CHECK(a && b && out, "pso_gemm_batched: null operand");
  PSO_ARG_CHECK(al16(a) && al16(b) && (lda % 8) == 0 && (ldb % 8) == 0 && (stride_a % 8) == 0 && (stride_b % 8) == 0,
                "pso_gemm_batched: A/B need 16-B aligned rows and batch strides");
  PSO_DTYPE_CHECK(out_dtype, "pso_gemm_batched");
  PSO_ARG_CHECK((long)M * lda < 0x7fffffffL && (long)N * ldb < 0x7fffffffL,
                "pso_gemm_batched: one operand spans more than 2^31 elements");
  GemmArgs g = batched_args(batch, M, N, K, a, lda, stride_a, b, ldb, stride_b, alpha, out, ldo, stride_o, out_dtype);
  return run_gemm(g, (hipStream_t)stream);
}

int pso_conv2d(int mode, int B, const void* src1, int C1, const void* src2, int C2, int H, int W, int Ho, int Wo,
               int ks, int stride, int pad, const void* weight, int Cout, const void* a2, long lda2, int K2,
               const void* b2, long ldb2, float alpha, const void* bias, const void* rowbias, long ld_rowbias,
               const void* resid, long ldr, void* out, long ldo, int out_dtype, int accumulate, void* stream) {
  GemmArgs g{};
  const int rc = conv_entry_args("pso_conv2d", g, mode, B, src1, C1, src2, C2, H, W, Ho, Wo, ks, stride, pad, weight,
                                 Cout, a2, lda2, K2, b2, ldb2, alpha, bias, rowbias, ld_rowbias, resid, ldr, out, ldo,
                                 out_dtype, accumulate);
  // only this entry takes the direct small-Cout convolution (gemm_plan.h GF_SMALL_CONV)
  return rc != PSO_OK ? rc : run_gemm(g, (hipStream_t)stream, 0, alpha == 1.f && ldo == Cout);
}

size_t pso_conv2d_ws_bytes(int B, int Ho, int Wo, int Cout, int K1, int K2) {
  const long M = (long)B * Ho * Wo;
  if (M <= 0 || M > 0x7fffffffL) return 0;
  return pso_gemm_ws_bytes((int)M, Cout, K1, K2);
}

// the workspace form applies when the plan splits and the workspace holds every split; else the plain conv
int pso_conv2d_ws(int mode, int B, const void* src1, int C1, const void* src2, int C2, int H, int W, int Ho, int Wo,
                  int ks, int stride, int pad, const void* weight, int Cout, const void* a2, long lda2, int K2,
                  const void* b2, long ldb2, float alpha, const void* bias, const void* rowbias, long ld_rowbias,
                  const void* resid, long ldr, void* out, long ldo, int out_dtype, int accumulate, void* ws,
                  size_t ws_bytes, void* stream) {
  GemmArgs g{};
  const int rc = conv_entry_args("pso_conv2d_ws", g, mode, B, src1, C1, src2, C2, H, W, Ho, Wo, ks, stride, pad, weight,
                                 Cout, a2, lda2, K2, b2, ldb2, alpha, bias, rowbias, ld_rowbias, resid, ldr, out, ldo,
                                 out_dtype, accumulate);
  g.ws = (float*)ws;
  return rc != PSO_OK ? rc : run_gemm(g, (hipStream_t)stream, ws_bytes);
}

int pso_gemm_geglu(int M, int N, const void* a, long lda, int K, const void* w, long ldw, const void* bias, void* out,
                   long ldo, void* out_pre, long ld_pre, int pre_rows, void* stream) {
  PSO_ARG_CHECK(M > 0 && N > 0 && (N % 256) == 0 && K > 0 && (K % 8) == 0 && a && w && bias && out,
                "pso_gemm_geglu: need N %% 256 == 0, K %% 8 == 0, bias");
  PSO_ARG_CHECK(al16(a) && al16(w) && (lda % 8) == 0 && (ldw % 8) == 0 && al16(out) && (ldo % 8) == 0 && al8(bias) &&
                    (!out_pre || (al16(out_pre) && (ld_pre % 8) == 0)),
                "pso_gemm_geglu: alignment (16-B rows)");
  PSO_ARG_CHECK((long)M * lda < 0x7fffffffL && (long)N * ldw < 0x7fffffffL, "pso_gemm_geglu: operand too large");
  GemmArgs g{};
  g.a1 = (const bf16_t*)a; g.lda1 = lda; g.K1 = K;
  g.b1 = (const bf16_t*)w; g.ldb1 = ldw;
  g.M = M; g.N = N; g.alpha = 1.f;
  g.bias = (const bf16_t*)bias;
  g.out = out; g.ldo = ldo; g.out_dtype = PSO_ELEM;
  g.out2 = out_pre; g.ldo2 = ld_pre;
  g.tail_m = (pre_rows > 0 && pre_rows < M) ? pre_rows : M;
  g.rows_per_group = 1;
  return run_plan(geglu_plan(M, N, K, lda == ldw, fits30(M, lda) && fits30(N, ldw), g_gemm_knobs), g,
                  (hipStream_t)stream);
}

int pso_gemm_geglu_bwd(int M, int N, const void* a, long lda, int K, const void* w, long ldw, const void* pre,
                       long ld_pre, void* out, long ldo, void* stream) {
  PSO_ARG_CHECK(M > 0 && N > 0 && (N % 32) == 0 && K > 0 && (K % 8) == 0 && a && w && pre && out,
                "pso_gemm_geglu_bwd: need N %% 32 == 0, K %% 8 == 0");
  PSO_ARG_CHECK(al16(a) && al16(w) && (lda % 8) == 0 && (ldw % 8) == 0 && al16(out) && (ldo % 8) == 0 && al16(pre) &&
                    (ld_pre % 8) == 0,
                "pso_gemm_geglu_bwd: alignment (16-B rows)");
  PSO_ARG_CHECK((long)M * lda < 0x7fffffffL && (long)N * ldw < 0x7fffffffL, "pso_gemm_geglu_bwd: operand too large");
  GemmArgs g{};
  g.a1 = (const bf16_t*)a; g.lda1 = lda; g.K1 = K;
  g.b1 = (const bf16_t*)w; g.ldb1 = ldw;
  g.M = M; g.N = N; g.alpha = 1.f;
  g.out = out; g.ldo = ldo; g.out_dtype = PSO_ELEM;
  g.aux = (const bf16_t*)pre; g.ldaux = ld_pre;
  g.rows_per_group = 1;
  return run_plan(geglu_bwd_plan(M, N, K, lda == ldw, fits30(M, lda) && fits30(N, ldw), g_gemm_knobs), g,
                  (hipStream_t)stream);
}

#ifdef PSO_BENCH_KNOBS
void pso_gemm_set_variant(int v) {
  g_gemm_knobs.variant = v % 100;
  g_gemm_knobs.group = v / 100;
}
void pso_gemm_tn_set_split(int ks) { g_gemm_knobs.tn_split = ks; }

static const void* plan_query_ptr(int align) { return align > 0 ? (const void*)(uintptr_t)(0x10000 + (align & 15)) : nullptr; }

// gemm_plan.h's answer for a problem given by value (include/pso_amd_knobs.h): the entries' own argument checks and
// fillers run on stand-in addresses of the given alignment, which are never dereferenced; nothing is launched
int pso_gemm_plan_query(int kind, const PsoGemmPlanQuery* q, PsoGemmPlanInfo* info) {
  PSO_ARG_CHECK(q && info, "pso_gemm_plan_query: null argument");
  GemmKnobs k;
  k.variant = q->variant; k.group = q->group; k.tn_split = q->tn_split;
  const void* const op = plan_query_ptr(16);
  void* const out = (void*)plan_query_ptr(q->out_align);
  const void *bias = plan_query_ptr(q->bias_align), *rowbias = plan_query_ptr(q->rowbias_align),
             *resid = plan_query_ptr(q->resid_align), *tail = q->K2 > 0 ? op : nullptr;
  *info = PsoGemmPlanInfo{};
  GemmPlan p;
  GemmArgs g{};
  bool small_conv_entry = false;
  switch (kind) {
    case PSO_PLAN_GEMM: {
      const int rc = gemm_entry_args("pso_gemm_plan_query", g, q->M, q->N, op, q->lda1, q->K1, op, q->ldb1, tail,
                                     q->lda2, q->K2, tail, q->ldb2, q->alpha, bias, rowbias, q->ld_rowbias,
                                     q->rows_per_group, resid, q->ldr, out, q->ldo, q->out_dtype, q->accumulate,
                                     q->tail_group_n, q->tail_rows);
      if (rc != PSO_OK) return rc;
      break;
    }
    case PSO_PLAN_CONV: {
      const int rc = conv_entry_args("pso_gemm_plan_query", g, q->conv_mode, q->B, op, q->C1, q->C2 ? op : nullptr,
                                     q->C2, q->H, q->W, q->Ho, q->Wo, q->ks, q->stride, q->pad, op, q->N, tail, q->lda2,
                                     q->K2, tail, q->ldb2, q->alpha, bias, rowbias, q->ld_rowbias, resid, q->ldr, out,
                                     q->ldo, q->out_dtype, q->accumulate);
      if (rc != PSO_OK) return rc;
      small_conv_entry = !q->have_ws && q->alpha == 1.f && q->ldo == q->N;
      break;
    }
    case PSO_PLAN_BATCHED:
      g = batched_args(q->batch, q->M, q->N, q->K1, op, q->lda1, 0, op, q->ldb1, 0, q->alpha, out, q->ldo, 0,
                       q->out_dtype);
      break;
    case PSO_PLAN_GEGLU:
    case PSO_PLAN_GEGLU_BWD: {
      const bool fits = fits30(q->M, q->lda1) && fits30(q->N, q->ldb1);
      p = kind == PSO_PLAN_GEGLU ? geglu_plan(q->M, q->N, q->K1, q->lda1 == q->ldb1, fits, k)
                                 : geglu_bwd_plan(q->M, q->N, q->K1, q->lda1 == q->ldb1, fits, k);
      break;
    }
    case PSO_PLAN_TN:
    case PSO_PLAN_TN_GEGLU: {
      const TnPlan t = kind == PSO_PLAN_TN_GEGLU
                           ? tn_geglu_plan(q->M, q->N, q->K1, q->lda1, q->ldb1, k)
                           : tn_plan(q->M, q->N, q->K1, q->lda1, q->ldb1, q->tn_group, q->have_ws != 0, k);
      info->form = t.kind;
      info->ws_ks = t.ws ? t.ks : 0;
      info->atomic_ks = t.ws ? 1 : t.ks;
      return PSO_OK;
    }
    default: PSO_ARG_CHECK(false, "pso_gemm_plan_query: bad kind %d", kind);
  }
  if (kind <= PSO_PLAN_BATCHED) {
    g.ws = q->have_ws ? (float*)op : nullptr;
    p = gemm_plan(gemm_facts(g, q->have_ws ? ~(size_t)0 : 0, small_conv_entry), k);
  }
  info->form = p.form; info->bm = p.BM; info->bn = p.BN; info->wm = p.WM; info->wn = p.WN; info->stages = p.STAGES;
  info->pipe = p.PIPE; info->epi = p.epi; info->conv_mode = p.form == GF_TILE && p.epi == GEPI_NONE ? g.conv.mode : 0;
  info->atomic_ks = p.atomic_ks; info->ws_ks = p.ws_ks;
  info->stage_epi = p.stage_epi; info->vec_ok = p.vec_ok; info->group_m = p.group_m;
  return PSO_OK;
}
#endif

int pso_gemm_skinny_grouped(int M, int N, int K, const void* A, long lda, const void* W, long ldw, float alpha,
                            void* out, long ldo, int groups, void* stream) {
  PSO_ARG_CHECK(M > 0 && N > 0 && N <= 128 && (N % 4) == 0 && K > 0 && (K % 8) == 0 && groups >= 1 && A && W && out,
                "pso_gemm_skinny_grouped: need 0 < N <= 128, N %% 4 == 0, K %% 8 == 0");
  PSO_ARG_CHECK(al16(A) && al16(W) && (lda % 8) == 0 && (ldw % 8) == 0 && al8(out) && (ldo % 4) == 0,
                "pso_gemm_skinny_grouped: alignment");
  return pso_gemm_skinny_nt(M, N, K, A, lda, W, ldw, alpha, out, ldo, 0, 0, groups, (hipStream_t)stream);
}

int pso_gemm_tn(int M, int I, int J, const void* A, long lda, const void* B, long ldb, float alpha, float* out,
                long ldo, void* stream) {
  return pso_gemm_tn_grouped(M, I, J, A, lda, B, ldb, alpha, out, ldo, 0, stream);
}

int pso_gemm_tn_grouped(int M, int I, int J, const void* A, long lda, const void* B, long ldb, float alpha, float* out,
                        long ldo, int group, void* stream) {
  PSO_ARG_CHECK(M >= 0 && I > 0 && J > 0 && A && B && out, "pso_gemm_tn: bad args");
  PSO_ARG_CHECK(al16(A) && al16(B) && (lda % 8) == 0 && (ldb % 8) == 0 && (I % 8) == 0 && (J % 8) == 0,
                "pso_gemm_tn: operands need 16-B aligned rows and I, J multiples of 8");
  if (M == 0) return PSO_OK;
  const TnPlan p = tn_plan(M, I, J, lda, ldb, group, false, g_gemm_knobs);
  if (p.kind == TNP_RANK)
    return p.swap ? pso_gemm_tn_rank(M, J, B, ldb, A, lda, p.rank, 0, alpha, out, ldo, 1, (hipStream_t)stream)
                  : pso_gemm_tn_rank(M, I, A, lda, B, ldb, p.rank, group, alpha, out, ldo, 0, (hipStream_t)stream);
  PSO_ARG_CHECK(p.kind != TNP_BAD_GROUP, "pso_gemm_tn: grouped form needs a rank-32/64/96 side and 128 | group");
  tn_launch_tiles(p, M, I, J, A, lda, B, ldb, alpha, out, ldo, nullptr, (hipStream_t)stream);
  return pso_check_launch("pso_gemm_tn");
}

int pso_gemm_tn_geglu(int M, int F2, int J, const void* A, long lda, const void* B, long ldb, float alpha, float* out,
                      long ldo, void* stream) {
  PSO_ARG_CHECK(M >= 0 && F2 > 0 && (F2 % 128) == 0 && J >= 128 && (J % 8) == 0 && A && B && out,
                "pso_gemm_tn_geglu: need 128 | F2 (F2=%d), J >= 128, 8 | J (J=%d)", F2, J);
  PSO_ARG_CHECK(al16(A) && al16(B) && (lda % 8) == 0 && (ldb % 8) == 0, "pso_gemm_tn_geglu: 16-B aligned rows");
  PSO_ARG_CHECK((long)M * lda < (1L << 30) && (long)M * ldb < (1L << 30), "pso_gemm_tn_geglu: operand too large");
  if (M == 0) return PSO_OK;
  const TnPlan p = tn_geglu_plan(M, F2, J, lda, ldb, g_gemm_knobs);
  if (p.kind == TNP_256) {
    tn256_launch(M, F2, J, A, lda, B, ldb, alpha, out, ldo, 1, nullptr, F2 / 2, (hipStream_t)stream);
    return pso_check_launch("pso_gemm_tn_geglu");
  }
  const int t128 = (F2 / 128) * ((J + 127) / 128);
  pso_note_kernel("gemm_tn128_kernel");
  gemm_tn128_kernel<<<dim3(t128, 1), 256, 0, (hipStream_t)stream>>>(M, F2, J, (const bf16_t*)A, lda, (const bf16_t*)B,
                                                                     ldb, alpha, out, ldo, p.steps, nullptr, F2 / 2);
  return pso_check_launch("pso_gemm_tn_geglu");
}

}  // extern "C"
