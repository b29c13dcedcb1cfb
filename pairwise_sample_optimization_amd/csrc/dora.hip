// DoRA (weight-decomposed LoRA, peft 0.11 DoraLinearLayer) around the existing LoRA projections:
//   n_j = || W_j + s (B A)_j ||_2   (row-wise over `in`, no gradient flows through it),  g_j = m_j / n_j
//   y   = g . z (+ bias) (+ resid)  with z = x W^T + s (x A^T) B^T, what the GEMM + LoRA K-tail computes
//   dy_g = g . dy  (feeds the unchanged LoRA backward),  dm_j += (1 / n_j) sum_rows dy[row, j] z[row, j]
// Three entries, none of which touches a GEMM:
//   pso_dora_weight_norm: ONE launch over a device descriptor table (one record per peft tensor) that reads the 16-bit
//                         base weight and the fp32 LoRA masters in peft's shapes and writes n and g (and m := n at init)
//   pso_dora_scale_fwd:   the column scale with the bias / residual the GEMM epilogue would have added
//   pso_dora_bwd:         dy_g out of place + the magnitude gradient, reduced in two stages in a fixed order
// fp32 arithmetic throughout, no float atomics: two runs give the same bits.  There is no epsilon in m / n (peft has
// none): a zero row of W + s B A gives inf here as there.
#include "common.h"

struct DoraNormDesc {  // 72 bytes, mirrored by kernels.DoraNormTable
  const bf16_t* W;     // [out][in] 16-bit base weight rows, row stride ldw (8-B aligned rows)
  const float* A;      // [r][in] fp32 master, rows contiguous (16-B aligned)
  const float* B;      // [out][r] fp32 master, rows contiguous (any 4-B boundary)
  float* m;            // [out] magnitude master (read; written in init mode)
  float* n;            // [out] row norms
  float* g;            // [out] m / n
  long ldw;
  int out, in, r;
  float s;             // alpha / r
};

#define DORA_NORM_ROWS 4                       // rows per wave: A's columns are loaded once for all of them
#define DORA_NORM_BLOCK_ROWS (4 * DORA_NORM_ROWS)  // 4 waves per block

// One wave owns DORA_NORM_ROWS rows.  A lane takes 4 consecutive columns at a time (one 8-B load of W, one 16-B load
// of each A row), columns lane * 4 + 256 * t in ascending t; it squares W + s sum_k B A per element (never
// n^2 = |W|^2 + 2 s W.BA + ...: the cross terms cancel) and adds the squares to its own partial sum.  Stage two is the
// xor butterfly over the 64 lanes.  Both stages have a fixed order.
__global__ __launch_bounds__(256) void dora_weight_norm_kernel(const DoraNormDesc* __restrict__ d, int init) {
  const DoraNormDesc t = d[blockIdx.y];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int row0 = (blockIdx.x * 4 + wave) * DORA_NORM_ROWS; row0 < t.out; row0 += gridDim.x * DORA_NORM_BLOCK_ROWS) {
    float acc[DORA_NORM_ROWS];
#pragma unroll
    for (int i = 0; i < DORA_NORM_ROWS; ++i) acc[i] = 0.f;
    for (int c = lane * 4; c < t.in; c += 256) {
      float v[DORA_NORM_ROWS][4];
#pragma unroll
      for (int i = 0; i < DORA_NORM_ROWS; ++i) v[i][0] = v[i][1] = v[i][2] = v[i][3] = 0.f;
      for (int k = 0; k < t.r; ++k) {
        const float4 a = *reinterpret_cast<const float4*>(t.A + (long)k * t.in + c);
#pragma unroll
        for (int i = 0; i < DORA_NORM_ROWS; ++i) {
          const int row = row0 + i < t.out ? row0 + i : t.out - 1;  // clamped: the surplus rows are not stored
          const float b = t.B[(long)row * t.r + k];
          v[i][0] += b * a.x, v[i][1] += b * a.y, v[i][2] += b * a.z, v[i][3] += b * a.w;
        }
      }
#pragma unroll
      for (int i = 0; i < DORA_NORM_ROWS; ++i) {
        const int row = row0 + i < t.out ? row0 + i : t.out - 1;
        const uint2 w = *reinterpret_cast<const uint2*>(t.W + (long)row * t.ldw + c);
        const float e0 = bf2f((bf16_t)(w.x & 0xffff)) + t.s * v[i][0], e1 = bf2f((bf16_t)(w.x >> 16)) + t.s * v[i][1];
        const float e2 = bf2f((bf16_t)(w.y & 0xffff)) + t.s * v[i][2], e3 = bf2f((bf16_t)(w.y >> 16)) + t.s * v[i][3];
        acc[i] += e0 * e0, acc[i] += e1 * e1, acc[i] += e2 * e2, acc[i] += e3 * e3;
      }
    }
#pragma unroll
    for (int i = 0; i < DORA_NORM_ROWS; ++i) {
      const float nn = sqrtf(warp_sum(acc[i]));
      const int row = row0 + i;
      if (lane == 0 && row < t.out) {
        const float mm = init ? nn : t.m[row];
        if (init) t.m[row] = nn;
        t.n[row] = nn;
        t.g[row] = mm / nn;
      }
    }
  }
}

// one item = 8 consecutive columns of one row: one 16-B load of z (and of resid), one 16-B store
__global__ __launch_bounds__(256) void dora_scale_fwd_kernel(int M, int N, int rows_policy, const bf16_t* __restrict__ z,
                                                             long ldz, const float* __restrict__ g,
                                                             const bf16_t* __restrict__ bias,
                                                             const bf16_t* __restrict__ resid, long ldr,
                                                             bf16_t* __restrict__ y, long ldy) {
  const int cg = N >> 3;
  const long items = (long)M * cg;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < items; i += (long)gridDim.x * blockDim.x) {
    const int row = (int)(i / cg), c0 = (int)(i - (long)row * cg) << 3;
    const uint4 zv = *reinterpret_cast<const uint4*>(z + (long)row * ldz + c0);
    const uint32_t zu[4] = {zv.x, zv.y, zv.z, zv.w};
    float v[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[2 * j] = bf2f((bf16_t)(zu[j] & 0xffff)), v[2 * j + 1] = bf2f((bf16_t)(zu[j] >> 16));
    if (row < rows_policy) {  // the rows past it are the adapter-free reference half of a paired pass
      const float4 g0 = *reinterpret_cast<const float4*>(g + c0), g1 = *reinterpret_cast<const float4*>(g + c0 + 4);
      v[0] *= g0.x, v[1] *= g0.y, v[2] *= g0.z, v[3] *= g0.w, v[4] *= g1.x, v[5] *= g1.y, v[6] *= g1.z, v[7] *= g1.w;
    }
    if (bias) {
      const uint4 bv = *reinterpret_cast<const uint4*>(bias + c0);
      const uint32_t bu[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        v[2 * j] += bf2f((bf16_t)(bu[j] & 0xffff)), v[2 * j + 1] += bf2f((bf16_t)(bu[j] >> 16));
    }
    if (resid) {
      const uint4 rv = *reinterpret_cast<const uint4*>(resid + (long)row * ldr + c0);
      const uint32_t ru[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        v[2 * j] += bf2f((bf16_t)(ru[j] & 0xffff)), v[2 * j + 1] += bf2f((bf16_t)(ru[j] >> 16));
    }
    *reinterpret_cast<uint4*>(y + (long)row * ldy + c0) =
        make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7]));
  }
}

#define DORA_BWD_ROWS 64  // rows per block of the first reduction stage

// Stage one: a block owns DORA_BWD_ROWS rows x 256 columns; thread (ty, tx) walks the rows ty, ty + 8, ... of the
// slab for the 8 columns of tx, writes dy_g and keeps sum dy z in registers; the 8 row groups are then added through
// LDS in ascending ty and the slab's column sums go to the workspace as part[slab][N].
__global__ __launch_bounds__(256) void dora_bwd_kernel(int M, int N, const bf16_t* __restrict__ dy, long lddy,
                                                       const bf16_t* __restrict__ z, long ldz,
                                                       const float* __restrict__ g, bf16_t* __restrict__ dyg,
                                                       long lddyg, float* __restrict__ part) {
  __shared__ float red[8][32][9];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c0 = (blockIdx.x * 32 + tx) << 3;
  const int r0 = blockIdx.y * DORA_BWD_ROWS;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c0 < N) {
    const float4 g0 = *reinterpret_cast<const float4*>(g + c0), g1 = *reinterpret_cast<const float4*>(g + c0 + 4);
    const float gs[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
    const int r1 = r0 + DORA_BWD_ROWS < M ? r0 + DORA_BWD_ROWS : M;
    for (int row = r0 + ty; row < r1; row += 8) {
      const uint4 dv = *reinterpret_cast<const uint4*>(dy + (long)row * lddy + c0);
      const uint4 zv = *reinterpret_cast<const uint4*>(z + (long)row * ldz + c0);
      const uint32_t du[4] = {dv.x, dv.y, dv.z, dv.w}, zu[4] = {zv.x, zv.y, zv.z, zv.w};
      float o[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d0 = bf2f((bf16_t)(du[j] & 0xffff)), d1 = bf2f((bf16_t)(du[j] >> 16));
        acc[2 * j] += d0 * bf2f((bf16_t)(zu[j] & 0xffff));
        acc[2 * j + 1] += d1 * bf2f((bf16_t)(zu[j] >> 16));
        o[2 * j] = gs[2 * j] * d0, o[2 * j + 1] = gs[2 * j + 1] * d1;
      }
      *reinterpret_cast<uint4*>(dyg + (long)row * lddyg + c0) =
          make_uint4(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]), pack2bf(o[4], o[5]), pack2bf(o[6], o[7]));
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[ty][tx][j] = acc[j];
  __syncthreads();
  // 256 threads = 32 column groups x 8 columns: thread t sums column (t >> 3, t & 7) over the 8 row groups
  const int sx = threadIdx.x >> 3, sj = threadIdx.x & 7;
  const int col = ((blockIdx.x * 32 + sx) << 3) + sj;
  if (col < N) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += red[k][sx][sj];
    part[(long)blockIdx.y * N + col] = s;
  }
}

// Stage two: dm_j += (1 / n_j) * (part[0][j] + part[1][j] + ...), slabs in ascending order
__global__ __launch_bounds__(256) void dora_dm_kernel(int N, int slabs, const float* __restrict__ part,
                                                      const float* __restrict__ n, float* __restrict__ dm) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= N) return;
  float s = 0.f;
  for (int k = 0; k < slabs; ++k) s += part[(long)k * N + j];
  dm[j] += s / n[j];
}

static bool dora_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" {

int pso_dora_weight_norm(int n, const void* descs, int max_out, int init, void* stream) {
  PSO_ARG_CHECK(n > 0 && n <= 65535 && descs && max_out > 0, "pso_dora_weight_norm: bad args");
  int bx = cdiv(max_out, DORA_NORM_BLOCK_ROWS);
  if (bx > 128) bx = 128;  // grid-stride beyond that
  dora_weight_norm_kernel<<<dim3((unsigned)bx, (unsigned)n, 1), 256, 0, (hipStream_t)stream>>>(
      (const DoraNormDesc*)descs, init != 0);
  return pso_check_launch("pso_dora_weight_norm");
}

int pso_dora_scale_fwd(int M, int N, int rows_policy, const void* z, long ldz, const float* g, const void* bias,
                       const void* resid, long ldr, void* y, long ldy, void* stream) {
  PSO_ARG_CHECK(M > 0 && N > 0 && rows_policy >= 0 && rows_policy <= M && z && g && y,
                "pso_dora_scale_fwd: bad args (M=%d N=%d rows_policy=%d)", M, N, rows_policy);
  PSO_ARG_CHECK(N % 8 == 0 && ldz % 8 == 0 && ldy % 8 == 0 && ldz >= N && ldy >= N && dora_al16(z) && dora_al16(y) &&
                    dora_al16(g) && dora_al16(bias) && dora_al16(resid) && (!resid || (ldr % 8 == 0 && ldr >= N)),
                "pso_dora_scale_fwd: z, g, bias, resid and y need 16-B aligned rows (N %% 8 == 0, ld %% 8 == 0)");
  long blocks = ((long)M * (N / 8) + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  dora_scale_fwd_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(
      M, N, rows_policy, (const bf16_t*)z, ldz, g, (const bf16_t*)bias, (const bf16_t*)resid, ldr, (bf16_t*)y, ldy);
  return pso_check_launch("pso_dora_scale_fwd");
}

size_t pso_dora_bwd_ws_bytes(int M, int N) {
  if (M <= 0 || N <= 0) return 0;
  return (size_t)cdiv(M, DORA_BWD_ROWS) * (size_t)N * sizeof(float);
}

int pso_dora_bwd(int M, int N, const void* dy, long lddy, const void* z, long ldz, const float* g, const float* n,
                 void* dyg, long lddyg, float* dm, void* ws, size_t ws_bytes, void* stream) {
  PSO_ARG_CHECK(M > 0 && N > 0 && dy && z && g && n && dyg && dm && ws, "pso_dora_bwd: bad args (M=%d N=%d)", M, N);
  PSO_ARG_CHECK(N % 8 == 0 && lddy % 8 == 0 && ldz % 8 == 0 && lddyg % 8 == 0 && lddy >= N && ldz >= N &&
                    lddyg >= N && dora_al16(dy) && dora_al16(z) && dora_al16(dyg) && dora_al16(g),
                "pso_dora_bwd: dy, z, g and dy_g need 16-B aligned rows (N %% 8 == 0, ld %% 8 == 0)");
  PSO_ARG_CHECK((reinterpret_cast<uintptr_t>(ws) & 3) == 0 && ws_bytes >= pso_dora_bwd_ws_bytes(M, N),
                "pso_dora_bwd: workspace of %zu bytes, needs %zu", ws_bytes, pso_dora_bwd_ws_bytes(M, N));
  const int slabs = cdiv(M, DORA_BWD_ROWS);
  dora_bwd_kernel<<<dim3((unsigned)cdiv(N, 256), (unsigned)slabs, 1), 256, 0, (hipStream_t)stream>>>(
      M, N, (const bf16_t*)dy, lddy, (const bf16_t*)z, ldz, g, (bf16_t*)dyg, lddyg, (float*)ws);
  int rc = pso_check_launch("pso_dora_bwd");
  if (rc) return rc;
  dora_dm_kernel<<<(unsigned)cdiv(N, 256), 256, 0, (hipStream_t)stream>>>(N, slabs, (const float*)ws, n, dm);
  return pso_check_launch("pso_dora_bwd (dm)");
}

}  // extern "C"
