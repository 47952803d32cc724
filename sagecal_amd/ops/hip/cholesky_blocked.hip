// Blocked damped-Cholesky solve for large n on gfx950, fp32:
//   dp = (JtJ + mu*I)^-1 Jtr   per problem, 32 <= n <= MAXN_CHOL_XL.
//
// Third path over the device helpers of cholesky.hip (included before this
// file), for the joint cross-cluster normal equations (Pb = 8*M*N = 5120 at
// 64 stations x 10 clusters, above MAXN_CHOL_MW). The k_cholmw_* sequence
// is built for latency at n = 512: rank-32 trailing updates read straight
// from global memory rewrite the lower trailing matrix n/32 times, about
// 8*n^3/(6*32) bytes (5.6 GB per problem at n = 5120) in 2*n/32 launches.
// Here the factorisation is two-level right-looking with an outer block of
// XB = 128 columns: the trailing matrix is rewritten n/128 times, by
// LDS-tiled rank-128 MFMA updates in which every operand element is read
// from global memory once per 128x128 tile, and the 32-wide helpers work
// inside the outer block, out of LDS.
//
// Kernel sequence on one stream (plain launches, graph-capturable), 3 per
// outer block k plus 2:
//   k_cholmw_init   — reused as it is: L := A + mu*I, dp := b
//   k_cholxl_diag   — 1 WG/problem. The XB x XB diagonal block sits in LDS
//                     as four 32-column panels [XB][PST] (72 KB) and is
//                     factored left-looking: panel j is updated by MFMA from
//                     panels 0..j-1, its 32x32 block factored
//                     wave-synchronously, its rows below solved; then this
//                     block's step of the forward substitution. Writes L_kk
//                     (reciprocal pivots on the diagonal) to L and L^T.
//   k_cholxl_trsm   — grid = batch x strips of XS = 64 rows of the panel
//                     below the block. L_kk and the strip in LDS (108 KB);
//                     X L_kk^T = A_strip in four 32-column steps: MFMA
//                     update from the columns already solved (one 16x16
//                     tile per wave, 8 waves = 64 x 32), then rowsolve32.
//                     Writes the strip to the L^T mirror only (all that the
//                     update and the backward pass read) and subtracts
//                     strip . y_k from its own rows of dp.
//   k_cholxl_syrk   — one 256-thread WG per 128x128 tile of the lower
//                     triangle of the trailing tile grid; each of 4 waves
//                     owns a 64x64 quadrant as 4x4 fragments of
//                     mfma_f32_16x16x4f32 (64 accumulators). K = 128 runs
//                     through LDS in slices of XK = 16 rows of L^T, double
//                     buffered (36 KB), row stride XB + 16 so that the four
//                     K rows of a fragment fall on disjoint banks. The tile
//                     of L is read, updated and written once. Edge tiles
//                     are masked. On diagonal tiles the quadrant above the
//                     diagonal is not computed.
//   k_cholmw_subst  — reused: backward substitution over L^T, NaN poison.
//
// XS = 64 rather than 128: rowsolve32 runs one row per lane, so a strip
// keeps one wave busy in the solve whatever its height, and the shorter
// strip gives twice the workgroups (78 per problem at n = 5120) for the
// same LDS-resident L_kk. Compiler resource report for gfx950
// (-Rpass-analysis=kernel-resource-usage; scratch 0 and no VGPR spill in
// all three): diag 166 VGPRs, 74,000 B LDS (194 SGPRs held in VGPR lanes,
// like k_chol_solve's 412); trsm 60 VGPRs, 111,616 B LDS; syrk 72 VGPRs +
// 64 AGPRs (the accumulators), 36,864 B LDS, 3 waves/SIMD.
//
// Contract as in cholesky.hip: n a multiple of NB (NOT of XB: every kernel
// takes a ragged last block of 32, 64 or 96), scratch 2*n*n floats per
// problem (L | L^T), inputs untouched, a non-positive pivot sets
// info[problem] and poisons that problem's dp row only. No atomics on
// floats: every element of L, L^T and dp has one owning thread per launch
// and a fixed summation order.

#define XB 128                 // outer block
#define XP (XB / NB)           // 32-column panels per outer block
#define XS 64                  // trsm strip height
#define XPAN (XB * PST)        // floats in one LDS panel of XB rows
#define XK 16                  // K rows of L^T per syrk slice
#define XLD (XB + 16)          // syrk LDS row stride
#define XTH 256                // syrk workgroup
#define MAXN_CHOL_XL 16384

using xl_f32x4 = __attribute__((ext_vector_type(4))) float;

static inline size_t cholxl_diag_lds_bytes() {
  return (size_t)XP * XPAN * sizeof(float);
}
static inline size_t cholxl_trsm_lds_bytes() {
  return (size_t)XP * (XB + XS) * PST * sizeof(float);
}

// acc += P(rows ar of panels 0..j-1) . Q(rows bc of panels 0..j-1)^T over
// K = 32*j, one 16x16 fragment: lane (l15, l4) feeds row l15, K index l4
__device__ __forceinline__ xl_f32x4 xl_panel_mfma(
    const float* P, int pstride, int ar, const float* Q, int qstride, int bc,
    int j, int l4) {
  xl_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int p = 0; p < j; ++p) {
    const float* pa = P + p * pstride + ar * PST + l4;
    const float* qb = Q + p * qstride + bc * PST + l4;
#pragma unroll
    for (int kk = 0; kk < NB; kk += 4)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[kk], qb[kk], acc, 0, 0, 0);
  }
  return acc;
}

extern "C" __global__ void __launch_bounds__(NTH)
k_cholxl_diag(int n, int k, float* __restrict__ Lbuf, float* __restrict__ dp,
              int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float yv[NB];
  __shared__ float rdg[NB];
  __shared__ int bad;
  const int bid = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  float* L = Lbuf + (size_t)bid * 2 * n * n;
  float* LT = L + (size_t)n * n;
  float* xo = dp + (size_t)bid * n;
  const int nb = (n - k) < XB ? (n - k) : XB;   // 32, 64, 96 or 128
  const int np = nb / NB;
  if (tid == 0) bad = 0;
  // panel j holds columns 32j..32j+32 of the block, rows 32j..nb
  for (int j = 0; j < np; ++j)
    stage_rows<false>(smem + j * XPAN + j * NB * PST,
                      L + (size_t)(k + j * NB) * n + k + j * NB, n,
                      nb - j * NB, tid, 0.f);
  __syncthreads();
  for (int j = 0; j < np; ++j) {
    float* pj = smem + j * XPAN;
    const int r0 = j * NB;
    if (j > 0) {
      const int ntiles = ((nb - r0) >> 4) * 2;
      for (int tile = w; tile < ntiles; tile += NTH / 64) {
        const int I = tile >> 1, Jt = tile & 1;
        const xl_f32x4 acc = xl_panel_mfma(smem, XPAN, r0 + I * 16 + l15,
                                           smem, XPAN, r0 + Jt * 16 + l15,
                                           j, l4);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          pj[(r0 + I * 16 + l4 * 4 + reg) * PST + Jt * 16 + l15] -= acc[reg];
      }
      __syncthreads();
    }
    float* dg = pj + r0 * PST;
    if (tid < NB) factor_diag32<true>(dg, yv, rdg, &bad, tid);
    __syncthreads();
    for (int r = r0 + NB + tid; r < nb; r += NTH) {
      float rw[NB];
      rowsolve32<true>(pj + r * PST, dg, rdg, rw);
    }
    __syncthreads();
    // forward substitution: y = L_jj^-1 xo on wave 0, then the rows below
    if (tid < 64) subst_diag32<false, true>(dg, yv, xo + k + r0, tid);
    __syncthreads();
    for (int r = r0 + NB + tid; r < nb; r += NTH)
      xo[k + r] -= dot32(pj + r * PST, yv);
    __syncthreads();
  }
  for (int j = 0; j < np; ++j) {
    const int r0 = j * NB, rows = nb - r0;
    const float* pj = smem + j * XPAN + r0 * PST;
    float* Lp = L + (size_t)(k + r0) * n + k + r0;
    for (int idx = tid; idx < rows * (NB / 4); idx += NTH) {
      const int r = idx >> 3, c4 = (idx & 7) << 2;
      *(float4*)(Lp + (size_t)r * n + c4) = *(const float4*)(pj + r * PST + c4);
    }
    write_LT(LT + (size_t)(k + r0) * n + k + r0, n, pj, rows, tid);
  }
  if (bad && tid == 0) atomicOr(&info[bid], 1);
}

// rows r0..r0+nr of the panel below the full diagonal block at k
extern "C" __global__ void __launch_bounds__(NTH)
k_cholxl_trsm(int n, int k, int nstrips, float* __restrict__ Lbuf,
              float* __restrict__ dp) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float rdg[XB];
  __shared__ float yk[XB];
  const int bid = blockIdx.x / nstrips, s = blockIdx.x % nstrips;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  float* L = Lbuf + (size_t)bid * 2 * n * n;
  float* LT = L + (size_t)n * n;
  float* xo = dp + (size_t)bid * n;
  const int r0 = k + XB + s * XS;
  const int nr = (n - r0) < XS ? (n - r0) : XS;   // 32 or 64
  float* lk = smem;                 // L_kk, panel j rows 32j..XB
  float* sp = smem + XP * XPAN;     // strip, XP panels [XS][PST]
  for (int j = 0; j < XP; ++j) {
    stage_rows<false>(lk + j * XPAN + j * NB * PST,
                      L + (size_t)(k + j * NB) * n + k + j * NB, n,
                      XB - j * NB, tid, 0.f);
    stage_rows<false>(sp + j * XS * PST, L + (size_t)r0 * n + k + j * NB, n,
                      nr, tid, 0.f);
  }
  if (tid < XB) {
    rdg[tid] = L[(size_t)(k + tid) * n + k + tid];   // 1/pivot, from diag
    yk[tid] = xo[k + tid];
  }
  __syncthreads();
  for (int j = 0; j < XP; ++j) {
    float* sj = sp + j * XS * PST;
    if (j > 0) {
      const int I = w >> 1, Jt = w & 1;     // NTH/64 waves = XS/16 x 2 tiles
      if (I * 16 < nr) {
        const xl_f32x4 acc = xl_panel_mfma(sp, XS * PST, I * 16 + l15,
                                           lk, XPAN, j * NB + Jt * 16 + l15,
                                           j, l4);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          sj[(I * 16 + l4 * 4 + reg) * PST + Jt * 16 + l15] -= acc[reg];
      }
      __syncthreads();
    }
    if (tid < nr) {
      float rw[NB];
      rowsolve32<true>(sj + tid * PST, lk + j * XPAN + j * NB * PST,
                       rdg + j * NB, rw);
    }
    __syncthreads();
  }
  for (int j = 0; j < XP; ++j)
    write_LT(LT + (size_t)(k + j * NB) * n + r0, n, sp + j * XS * PST, nr,
             tid);
  if (tid < nr) {
    float acc = 0.f;
    for (int j = 0; j < XP; ++j)
      acc += dot32(sp + (j * XS + tid) * PST, yk + j * NB);
    xo[r0 + tid] -= acc;
  }
}

// tile t of the lower triangle of the XB tile grid over rows/cols k+XB..n:
// L_tile -= P_I . P_J^T with P the panel just solved, read from L^T rows
// k..k+XB
extern "C" __global__ void __launch_bounds__(XTH)
k_cholxl_syrk(int n, int k, int ntiles, float* __restrict__ Lbuf) {
  __shared__ __attribute__((aligned(16))) float sA[2][XK * XLD];
  __shared__ __attribute__((aligned(16))) float sB[2][XK * XLD];
  const int bid = blockIdx.x / ntiles, t = blockIdx.x % ntiles;
  int I = (int)((sqrtf(8.0f * t + 1.0f) - 1.0f) * 0.5f + 1e-4f);
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  while (I * (I + 1) / 2 > t) --I;
  const int J = t - I * (I + 1) / 2;
  float* L = Lbuf + (size_t)bid * 2 * n * n;
  const float* LTk = L + (size_t)n * n + (size_t)k * n;
  const int r0 = k + XB + I * XB, c0 = k + XB + J * XB;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int wr = w >> 1, wc = w & 1;
  // a quadrant wholly above the diagonal is never read again
  const bool live = !(I == J && wc > wr);
  // loader: a slice is XK rows of XB/4 float4 per operand, 2 per thread
  const int lq = tid >> 5, li = (tid & 31) << 2;
  const bool inA = r0 + li < n, inB = c0 + li < n;   // n % 4 == 0
  const float4 zero = {0.f, 0.f, 0.f, 0.f};
  float4 va0, va1, vb0, vb1;
  xl_f32x4 acc[4][4];
#pragma unroll
  for (int fi = 0; fi < 4; ++fi)
#pragma unroll
    for (int fj = 0; fj < 4; ++fj) acc[fi][fj] = {0.f, 0.f, 0.f, 0.f};

#define XL_LOAD(q0)                                                        \
  {                                                                        \
    const float* row = LTk + (size_t)((q0) + lq) * n;                      \
    const float* row8 = row + (size_t)(XK / 2) * n;                        \
    va0 = inA ? *(const float4*)(row + r0 + li) : zero;                    \
    va1 = inA ? *(const float4*)(row8 + r0 + li) : zero;                   \
    vb0 = inB ? *(const float4*)(row + c0 + li) : zero;                    \
    vb1 = inB ? *(const float4*)(row8 + c0 + li) : zero;                   \
  }
#define XL_STORE(buf)                                                      \
  {                                                                        \
    *(float4*)(&sA[buf][lq * XLD + li]) = va0;                             \
    *(float4*)(&sA[buf][(lq + XK / 2) * XLD + li]) = va1;                  \
    *(float4*)(&sB[buf][lq * XLD + li]) = vb0;                             \
    *(float4*)(&sB[buf][(lq + XK / 2) * XLD + li]) = vb1;                  \
  }

  XL_LOAD(0)
  XL_STORE(0)
  __syncthreads();
  for (int s = 0; s < XB / XK; ++s) {
    const int buf = s & 1;
    if (s + 1 < XB / XK) { XL_LOAD((s + 1) * XK) }
    if (live) {
      const float* pa = &sA[buf][l4 * XLD + wr * 64 + l15];
      const float* pb = &sB[buf][l4 * XLD + wc * 64 + l15];
#pragma unroll
      for (int kk = 0; kk < XK; kk += 4) {
        float a[4], b[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          a[f] = pa[kk * XLD + f * 16];
          b[f] = pb[kk * XLD + f * 16];
        }
#pragma unroll
        for (int fi = 0; fi < 4; ++fi)
#pragma unroll
          for (int fj = 0; fj < 4; ++fj)
            acc[fi][fj] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                a[fi], b[fj], acc[fi][fj], 0, 0, 0);
      }
    }
    // the other buffer was last read before the barrier that ended the
    // previous slice
    if (s + 1 < XB / XK) { XL_STORE(buf ^ 1) }
    __syncthreads();
  }
#undef XL_LOAD
#undef XL_STORE
  if (!live) return;
  // D layout: col = lane&15, row = (lane>>4)*4 + reg
#pragma unroll
  for (int fi = 0; fi < 4; ++fi) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int r = r0 + wr * 64 + fi * 16 + l4 * 4 + reg;
      float* Lr = L + (size_t)r * n;
#pragma unroll
      for (int fj = 0; fj < 4; ++fj) {
        const int c = c0 + wc * 64 + fj * 16 + l15;
        if (r < n && c < n) Lr[c] -= acc[fi][fj][reg];
      }
    }
  }
}
