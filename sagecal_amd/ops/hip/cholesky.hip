// Batched damped-Cholesky solve for gfx950, fp32:
//   dp = (JtJ + mu*I)^-1 Jtr   per problem.
//
// Replaces rocSOLVER potrf/potrs for the LM normal equations (the
// reference used cusolverDn potrf/potrs per cluster, clmfit_cuda.c:364):
// rocSOLVER's batched fp32 potrf measures ~2 ms for [2,512,512] on MI355X,
// and the LM inner loop is a serial chain of such solves, so both paths
// here are built for low LATENCY at small batch.
//
// Two paths over one set of device helpers (32x32 diagonal factor, row
// solve, in-block substitution, panel staging, L^T write-back, damping):
//   k_chol_solve — one workgroup per problem, left-looking: each 32-column
//     panel is staged from the damped A into LDS (padded stride,
//     conflict-free float4), updated by MFMA from the L^T mirror of the
//     panels already factored, factored, and written back as L and L^T;
//     both substitutions follow in the same kernel.
//   k_cholmw_*   — right-looking kernel sequence that spreads the trailing
//     update over the whole chip (described further down).
// In both, the diagonal blocks are factored WAVE-SYNCHRONOUSLY in registers
// (lane r holds row r, no barriers), the substitutions are wave-synchronous
// in-block, and the backward pass reads rows of the L^T mirror (coalesced)
// instead of columns of L.
//
// Contract, enforced by the launchers: n is a multiple of NB (the host pads
// with an identity diagonal) and n <= MAXN_CHOL (fused) or MAXN_CHOL_MW
// (mw); every loop below relies on it. Lbuf scratch is 2*n*n floats per
// problem (L | L^T). A non-positive pivot is clamped, sets info[problem]
// and turns that problem's dp row into NaN; other problems are unaffected.
#include "common.h"

#define NB 32
#define PST 36   // padded LDS panel row stride (floats)
#define NTH 512
#define MAXN_CHOL 1024
// multi-workgroup path row-chunking: panels taller than PANEL_CAP rows
// stream through LDS in passes, lifting the mw size cap to MAXN_CHOL_MW
// (the 512-station 8N=4096 normal equations, clmfit_cuda.c:1624-1674)
#define PANEL_CAP 1024
#define MAXN_CHOL_MW 4096

// ---------------------------------------------------------------------
// Shared device helpers. RECIP selects the mw kernels' arithmetic
// (multiply by the stored reciprocal pivot) over the fused kernel's
// (divide by the pivot); the two round differently, so each path keeps
// its own.
// ---------------------------------------------------------------------

// add mu to whichever lane of the quad at (row, col..col+3) holds the
// diagonal; d = row - col
__device__ __forceinline__ void damp_diag(float4& v, int d, float m) {
  if (d >= 0 && d < 4) {
    if (d == 0) v.x += m;
    else if (d == 1) v.y += m;
    else if (d == 2) v.z += m;
    else v.w += m;
  }
}

// stage nr rows x NB cols from src (row stride n) into the LDS panel
// (float4); DAMP adds m on the diagonal of the block that src starts at
template <bool DAMP>
__device__ __forceinline__ void stage_rows(float* pan, const float* src,
                                           int n, int nr, int tid, float m) {
  for (int idx = tid; idx < nr * (NB / 4); idx += NTH) {
    const int r = idx >> 3, c4 = (idx & 7) << 2;
    float4 v = *(const float4*)(src + (size_t)r * n + c4);
    if (DAMP) damp_diag(v, r - c4, m);
    *(float4*)(pan + r * PST + c4) = v;
  }
}

// stage the lower (or, from the L^T mirror, UPPER) triangle of the 32x32
// diagonal block at (k, k) of M for the in-block substitution
template <bool UPPER>
__device__ __forceinline__ void stage_tri32(float* pan, const float* M,
                                            int n, int k, int tid) {
  for (int idx = tid; idx < NB * NB; idx += NTH) {
    const int r = idx >> 5, c = idx & 31;
    if (UPPER ? c >= r : c <= r)
      pan[r * PST + c] = M[(size_t)(k + r) * n + k + c];
  }
}

// wave-synchronous factor of the 32x32 block at the top of pan, called by
// lanes 0..31 of wave 0: lane r holds row r; the scaled pivot column is
// published through LDS (yv) once per step (in-wave LDS write->read
// ordering; broadcast reads are 1 cycle) — ~10x fewer DS ops than a
// shuffle-based rank-1 update. RECIP also leaves 1/pivot in rdg.
template <bool RECIP>
__device__ __forceinline__ void factor_diag32(float* pan, float* yv,
                                              float* rdg, int* bad, int r) {
  float row[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) row[c] = pan[r * PST + c];
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    // pivot broadcast via shfl (a divergent LDS write followed by a
    // uniform read is NOT ordered: the compiler emits the else-path
    // read before the taken-path write)
    float pivraw = __shfl(row[c], c, 64);
    if (pivraw <= 1e-30f) {
      if (r == 0) *bad = 1;
      pivraw = 1e-30f;
    }
    const float pv = sqrtf(pivraw);
    if (RECIP) {
      const float rpv = 1.0f / pv;
      if (r >= c) row[c] *= rpv;
      if (r == c) rdg[c] = rpv;
    } else {
      if (r >= c) row[c] /= pv;
    }
    yv[r] = row[c];              // non-divergent publish (one ds_write)
    const float lrc = row[c];
#pragma unroll
    for (int cc = c + 1; cc < NB; ++cc) {
      if (r >= cc) row[cc] -= lrc * yv[cc];
    }
  }
#pragma unroll
  for (int c = 0; c < NB; ++c) pan[r * PST + c] = row[c];
  // publish 1/pv on the panel diagonal: the LT mirror's diagonal is read
  // ONLY by the backward substitution's divide (syrk/fwd never touch it),
  // so storing the reciprocal there turns that divide into a multiply
  if (RECIP) pan[r * PST + r] = rdg[r];
}

// solve one sub-panel row in LDS against the factored diagonal block dg;
// the solved row is also left in rw. RECIP multiplies by the reciprocal
// diagonal: the 32 serial divides per row-thread were the panel's longest
// chain.
template <bool RECIP>
__device__ __forceinline__ void rowsolve32(float* prow, const float* dg,
                                           const float* rdg, float* rw) {
#pragma unroll
  for (int c = 0; c < NB; ++c) rw[c] = prow[c];
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    float s = rw[c];
#pragma unroll
    for (int c2 = 0; c2 < c; ++c2) s -= rw[c2] * dg[c * PST + c2];
    rw[c] = RECIP ? s * rdg[c] : s / dg[c * PST + c];
  }
#pragma unroll
  for (int c = 0; c < NB; ++c) prow[c] = rw[c];
}

// wave-synchronous substitution with the 32x32 triangle dg on wave 0 (all
// 64 lanes call it): xk[0..32) := T^-1 xk, also published in yv. Lower
// runs forward, UPPER backward. With RECIP the diagonal of dg holds the
// reciprocal pivot.
template <bool UPPER, bool RECIP>
__device__ __forceinline__ void subst_diag32(const float* dg, float* yv,
                                             float* xk, int lane) {
  const int r = lane & 31;
  float rv[NB];
  float bv = (lane < 32) ? xk[r] : 0.f;
  if (lane < 32) {
#pragma unroll
    for (int c = 0; c < NB; ++c)
      rv[c] = (UPPER ? c >= r : c <= r) ? dg[r * PST + c] : 0.f;
  }
#pragma unroll
  for (int ci = 0; ci < NB; ++ci) {
    const int c = UPPER ? NB - 1 - ci : ci;
    if (lane == c) {
      if (RECIP) bv *= rv[c];
      else bv /= rv[c];
    }
    const float xc = __shfl(bv, c, 64);
    if (lane < 32 && (UPPER ? r < c : r > c)) bv -= rv[c] * xc;
    if (lane == c) yv[c] = bv;
  }
  if (lane < 32) xk[r] = bv;
}

// row . yv over one block, c ascending: the rank-32 update of one entry of
// the right-hand side
__device__ __forceinline__ float dot32(const float* row, const float* yv) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NB; ++c) s += row[c] * yv[c];
  return s;
}

// L^T mirror write-back of nr panel rows; dst points at (column k, row
// k + r0) of LT. Writes are coalesced: r varies fastest within a column.
__device__ __forceinline__ void write_LT(float* dst, int n, const float* pan,
                                         int nr, int tid) {
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    for (int r = tid; r < nr; r += NTH) dst[(size_t)c * n + r] = pan[r * PST + c];
  }
}

// backward substitution L^T x = y in place in xo, reading LT rows
// (coalesced); pan holds one staged diagonal block
template <bool RECIP>
__device__ __forceinline__ void backward_subst(const float* LT, float* xo,
                                               int n, float* pan, float* yv,
                                               int tid) {
  for (int k = n - NB; k >= 0; k -= NB) {
    stage_tri32<true>(pan, LT, n, k, tid);
    __syncthreads();
    if (tid < 64) subst_diag32<true, RECIP>(pan, yv, xo + k, tid);
    __syncthreads();
    // update rows above: xo[i] -= LT[i, k..k+NB) . x[k..k+NB)  for i < k
    for (int i = tid; i < k; i += NTH) xo[i] -= dot32(LT + (size_t)i * n + k, yv);
    __syncthreads();
  }
}

__device__ __forceinline__ void poison_row(float* xo, int n, int tid) {
  const float qn = __int_as_float(0x7fc00000);
  for (int idx = tid; idx < n; idx += NTH) xo[idx] = qn;
}

// ======================================================================
// Fused single-kernel solver: one workgroup per problem.
// ======================================================================

// dynamic LDS of k_chol_solve: the first panel's n rows; the 40 further
// rows are never touched and stay so that the request, and with it the
// kernel's residency, is the one that was measured
static inline size_t chol_solve_lds_bytes(int n) {
  return (size_t)(n + 40) * PST * sizeof(float);
}

extern "C" __global__ void __launch_bounds__(NTH)
k_chol_solve(const float* __restrict__ JtJ, const float* __restrict__ Jtr,
             const float* __restrict__ mu, int n,
             float* __restrict__ Lbuf, float* __restrict__ dp,
             int* __restrict__ info) {
  const int bid = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const float* A = JtJ + (size_t)bid * n * n;
  float* L = Lbuf + (size_t)bid * 2 * n * n;       // [L | L^T] scratch
  float* LT = L + (size_t)n * n;
  const float* b = Jtr + (size_t)bid * n;
  float* xo = dp + (size_t)bid * n;

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* pan = smem;                  // [rows][PST]
  __shared__ float yv[NB];
  __shared__ int bad;

  // n >= NB, so the first panel's barriers order this before the factor's
  // write and every thread reads a settled flag at the end
  if (tid == 0) bad = 0;
  const float m = mu[bid];

  // no A->L copy: left-looking panels stage straight from the damped A;
  // L/LT only ever hold FACTORED panels.
  for (int k = 0; k < n; k += NB) {
    const int rows = n - k;
    stage_rows<true>(pan, A + (size_t)k * n + k, n, rows, tid, m);
    __syncthreads();
    // ---- LEFT-LOOKING update: S -= Lp(rows x k) * Lc(32 x k)^T
    // MFMA f32 16x16x4 (exact f32): both fragments load COALESCED from the
    // LT mirror (A[i][k'] = LT[k'][k+I16+i], B[k'][c] = LT[k'][k+c]) — one
    // dword per lane per operand per MFMA, ~6x fewer load-issue slots than
    // scalar float4 tiles, which are load-issue-bound on a single CU.
    if (k > 0) {
      const int w = tid >> 6;              // wave id (NTH/64 waves)
      const int l15 = lane & 15, l4 = lane >> 4;
      const int ntiles = (rows >> 4) * 2;  // 2 col-tiles of 16
      for (int tile = w; tile < ntiles; tile += NTH / 64) {
        const int I = tile >> 1, Jt = tile & 1;
        const int arow = k + I * 16 + l15;       // S row this lane loads
        const int bcol = k + Jt * 16 + l15;
        using f32x4 = __attribute__((ext_vector_type(4))) float;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float* LTb = LT + (size_t)l4 * n;  // + kk*n walks K
        // software-pipelined K loop: batch 4 MFMAs' loads ahead so L2
        // latency hides under the MFMA chain (k is a multiple of 32)
        for (int kk = 0; kk < k; kk += 16) {
          const float a0 = LTb[(size_t)kk * n + arow];
          const float a1 = LTb[(size_t)(kk + 4) * n + arow];
          const float a2 = LTb[(size_t)(kk + 8) * n + arow];
          const float a3 = LTb[(size_t)(kk + 12) * n + arow];
          const float b0 = LTb[(size_t)kk * n + bcol];
          const float b1 = LTb[(size_t)(kk + 4) * n + bcol];
          const float b2 = LTb[(size_t)(kk + 8) * n + bcol];
          const float b3 = LTb[(size_t)(kk + 12) * n + bcol];
          // all 8 loads issue before the first MFMA; left alone, the
          // scheduler sinks three of them between the MFMAs and waits
          // for each (3.9 ms instead of 2.5 ms at [2,1024,1024])
          __builtin_amdgcn_sched_group_barrier(0x020, 8, 0);  // VMEM reads
          __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);  // MFMAs
          acc =__builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, b2, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a3, b3, acc, 0, 0, 0);
        }
        // C/D layout: col = lane&15, row = (lane>>4)*4 + reg
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          pan[(I * 16 + l4 * 4 + reg) * PST + Jt * 16 + l15] -= acc[reg];
        }
      }
      __syncthreads();
    }
    if (tid < NB) factor_diag32<false>(pan, yv, nullptr, &bad, tid);
    __syncthreads();
    // row-solve sub-panel rows NB..rows against the diag block
    for (int r = NB + tid; r < rows; r += NTH) {
      float rw[NB];
      rowsolve32<false>(pan + r * PST, pan, nullptr, rw);
    }
    __syncthreads();
    // write panel back: L (row-major, float4) and the L^T mirror
    for (int idx = tid; idx < rows * (NB / 4); idx += NTH) {
      const int r = idx >> 3, c4 = (idx & 7) << 2;
      *(float4*)(L + (size_t)(k + r) * n + k + c4) =
          *(const float4*)(pan + r * PST + c4);
    }
    write_LT(LT + (size_t)k * n + k, n, pan, rows, tid);
    __syncthreads();
  }

  // ---- forward substitution: L y = b (y in xo) ----
  for (int idx = tid; idx < n; idx += NTH) xo[idx] = b[idx];
  __syncthreads();
  for (int k = 0; k < n; k += NB) {
    stage_tri32<false>(pan, L, n, k, tid);
    __syncthreads();
    if (tid < 64) subst_diag32<false, false>(pan, yv, xo + k, tid);
    __syncthreads();
    for (int i = k + NB + tid; i < n; i += NTH) xo[i] -= dot32(L + (size_t)i * n + k, yv);
    __syncthreads();
  }
  // ---- backward substitution: L^T x = y ----
  backward_subst<false>(LT, xo, n, pan, yv, tid);
  if (bad) {
    poison_row(xo, n, tid);
    if (tid == 0) atomicOr(&info[bid], 1);
  }
}

// ======================================================================
// Multi-workgroup right-looking variant.
//
// The single-kernel solver above runs ONE workgroup per problem: at the
// LM batch sizes of the headline config (B≈5, n=512) that is <2% of the
// 256 CUs and k_chol_solve measures ~65% of all GPU time (753 us/call,
// profiles/lm_kernel_stats_final.csv). Here the factorization is split
// into a kernel SEQUENCE on one stream (graph-captured, so launch cost
// is node dispatch only):
//   k_cholmw_init   — L := A + mu*I (working copy; right-looking mutates),
//                     dp := b
//   per panel k:
//     k_cholmw_panel — factor 32x32 diag + row-solve the panel + this
//                      panel's step of the forward substitution
//                      (1 WG/problem; serial critical path);
//                      k_cholmw_panel_big is the same body with row
//                      chunking for n > PANEL_CAP
//     k_cholmw_syrk  — trailing update: ONE 32x32 MFMA tile per 64-lane
//                      wave, grid = batch * n_lower_tiles — the O(n^3)
//                      work spreads over the whole chip instead of 1 CU
//   k_cholmw_subst  — backward substitution + NaN poison
// Same scratch contract as k_chol_solve (2*n*n: L | L^T mirror).
// ======================================================================

// grid (batch, SLICES): B workgroups alone leave the copy bandwidth-bound
// on B CUs (~75 us for [5,512,512]); sliced over 32 WGs/problem it is ~8 us.
// Also seeds dp := b (the panel kernels run the forward substitution
// in-place as each panel factors).
#define INIT_SLICES 32
extern "C" __global__ void __launch_bounds__(NTH)
k_cholmw_init(const float* __restrict__ JtJ, const float* __restrict__ Jtr,
              const float* __restrict__ mu, int n, float* __restrict__ Lbuf,
              float* __restrict__ dp) {
  const int bid = blockIdx.x, slice = blockIdx.y, tid = threadIdx.x;
  const float* A = JtJ + (size_t)bid * n * n;
  float* L = Lbuf + (size_t)bid * 2 * n * n;
  const float m = mu[bid];
  const int nq = n * n / 4;
  for (int idx = slice * NTH + tid; idx < nq; idx += NTH * INIT_SLICES) {
    const size_t p = 4ull * idx;
    float4 v = *(const float4*)(A + p);
    damp_diag(v, (int)(p / n) - (int)(p % n), m);
    *(float4*)(L + p) = v;
  }
  if (slice == 0) {
    for (int i = tid; i < n; i += NTH) dp[(size_t)bid * n + i] = Jtr[(size_t)bid * n + i];
  }
}

// dynamic LDS of the panel kernels: the single-pass kernel holds all n
// panel rows (+8 untouched rows, kept so the request stays the measured
// one); the chunked kernel holds PANEL_CAP rows and, behind them, the
// factored diagonal block
static inline size_t cholmw_panel_lds_bytes(int n) {
  const int rows = n <= PANEL_CAP ? n + 8 : PANEL_CAP + NB;
  return (size_t)rows * PST * sizeof(float);
}

// One panel of the right-looking factorization. CHUNKED keeps the factored
// 32x32 diag block resident at kept, so panels taller than the LDS budget
// (n > PANEL_CAP, up to MAXN_CHOL_MW) are processed in row passes: the
// row-solve/LT-writeback/fwd-subst of a row depend only on that block +
// rdg/yv, never on other rows. The single-pass kernel does not pay for the
// copy and its barrier.
template <bool CHUNKED>
__device__ __forceinline__ void cholmw_panel_body(
    int n, int k, float* Lbuf, float* dp, int* info, float* pan, float* kept,
    float* yv, float* rdg, int* bad) {
  const int bid = blockIdx.x, tid = threadIdx.x;
  float* L = Lbuf + (size_t)bid * 2 * n * n;
  float* LT = L + (size_t)n * n;
  float* xo = dp + (size_t)bid * n;
  if (tid == 0) *bad = 0;
  const int rows = n - k;
  const int cap = (CHUNKED && rows > PANEL_CAP) ? PANEL_CAP : rows;
  // stage panel rows k..k+cap, cols k..k+NB from the (already-updated) L
  const float* Lp = L + (size_t)k * n + k;
  float* LTp = LT + (size_t)k * n + k;
  stage_rows<false>(pan, Lp, n, cap, tid, 0.f);
  __syncthreads();
  if (tid < NB) factor_diag32<true>(pan, yv, rdg, bad, tid);
  __syncthreads();
  const float* dg = pan;
  if (CHUNKED) {
    for (int idx = tid; idx < NB * NB; idx += NTH) {
      const int r = idx >> 5, c = idx & 31;
      kept[r * PST + c] = pan[r * PST + c];
    }
    __syncthreads();
    dg = kept;
  }
  for (int r = NB + tid; r < cap; r += NTH) {
    float rw[NB];
    rowsolve32<true>(pan + r * PST, dg, rdg, rw);
  }
  __syncthreads();
  // write back the LT mirror ONLY: every consumer of the factored panel
  // (syrk fragments, fused forward subst via LDS, backward subst) reads
  // L^T; the L working copy keeps unfactored trailing values, which is
  // all that later panels ever stage.
  write_LT(LTp, n, pan, cap, tid);
  __syncthreads();
  // fused forward-substitution step: y_k = L_kk^-1 xo[k..k+NB] on wave 0,
  // then xo[k+NB..n] -= panel . y_k straight from LDS (the separate subst
  // kernel then only runs the backward pass)
  if (tid < 64) subst_diag32<false, true>(dg, yv, xo + k, tid);
  __syncthreads();
  for (int r = NB + tid; r < cap; r += NTH) xo[k + r] -= dot32(pan + r * PST, yv);
  if (CHUNKED) {
    // remaining row chunks (uniform trip count)
    for (int r0 = cap; r0 < rows; r0 += PANEL_CAP) {
      const int nr = (rows - r0) < PANEL_CAP ? (rows - r0) : PANEL_CAP;
      __syncthreads();
      stage_rows<false>(pan, Lp + (size_t)r0 * n, n, nr, tid, 0.f);
      __syncthreads();
      for (int r = tid; r < nr; r += NTH) {
        float rw[NB];
        rowsolve32<true>(pan + r * PST, dg, rdg, rw);
        xo[k + r0 + r] -= dot32(rw, yv);
      }
      __syncthreads();
      write_LT(LTp + r0, n, pan, nr, tid);
    }
  }
  if (*bad && tid == 0) atomicOr(&info[bid], 1);
}

extern "C" __global__ void __launch_bounds__(NTH)
k_cholmw_panel(int n, int k, float* __restrict__ Lbuf,
               float* __restrict__ dp, int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float yv[NB];
  __shared__ float rdg[NB];   // reciprocal diagonal (div -> mul downstream)
  __shared__ int bad;
  cholmw_panel_body<false>(n, k, Lbuf, dp, info, smem, nullptr, yv, rdg, &bad);
}

extern "C" __global__ void __launch_bounds__(NTH)
k_cholmw_panel_big(int n, int k, float* __restrict__ Lbuf,
                   float* __restrict__ dp, int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float yv[NB];
  __shared__ float rdg[NB];
  __shared__ int bad;
  cholmw_panel_body<true>(n, k, Lbuf, dp, info, smem, smem + PANEL_CAP * PST,
                          yv, rdg, &bad);
}

// trailing SYRK: tile t of the lower-triangular 32x32 tile grid of the
// trailing matrix (rows/cols k+NB..n). One 64-lane wave per tile: 2x2
// fragments of mfma_f32_16x16x4, K = NB, operands read COALESCED from
// the LT mirror (same fragment scheme as the left-looking update above).
extern "C" __global__ void __launch_bounds__(64)
k_cholmw_syrk(int n, int k, int ntiles, float* __restrict__ Lbuf) {
  const int g = blockIdx.x;
  const int bid = g / ntiles, t = g % ntiles;
  int I = (int)((sqrtf(8.0f * t + 1.0f) - 1.0f) * 0.5f + 1e-4f);
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  while (I * (I + 1) / 2 > t) --I;
  const int J = t - I * (I + 1) / 2;
  float* L = Lbuf + (size_t)bid * 2 * n * n;
  const float* LT = L + (size_t)n * n;
  const int r0 = k + NB + I * NB;
  const int c0 = k + NB + J * NB;
  const int lane = threadIdx.x & 63;
  const int l15 = lane & 15, l4 = lane >> 4;
  const float* LTb = LT + (size_t)(k + l4) * n;
  using f32x4 = __attribute__((ext_vector_type(4))) float;
  f32x4 a00 = {0.f, 0.f, 0.f, 0.f}, a01 = a00, a10 = a00, a11 = a00;
#pragma unroll
  for (int kk = 0; kk < NB; kk += 4) {
    const float x0 = LTb[(size_t)kk * n + r0 + l15];
    const float x1 = LTb[(size_t)kk * n + r0 + 16 + l15];
    const float y0 = LTb[(size_t)kk * n + c0 + l15];
    const float y1 = LTb[(size_t)kk * n + c0 + 16 + l15];
    a00 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0, y0, a00, 0, 0, 0);
    a01 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0, y1, a01, 0, 0, 0);
    a10 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1, y0, a10, 0, 0, 0);
    a11 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1, y1, a11, 0, 0, 0);
  }
  // D layout: col = lane&15, row = (lane>>4)*4 + reg
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int ra = r0 + l4 * 4 + reg, rb = ra + 16;
    const int ca = c0 + l15, cb = ca + 16;
    L[(size_t)ra * n + ca] -= a00[reg];
    L[(size_t)ra * n + cb] -= a01[reg];
    L[(size_t)rb * n + ca] -= a10[reg];
    L[(size_t)rb * n + cb] -= a11[reg];
  }
}

// backward substitution only: dp already holds y = L^-1 b (forward pass
// fused into the panel kernels); the LT diagonal holds 1/pv
extern "C" __global__ void __launch_bounds__(NTH)
k_cholmw_subst(int n, const float* __restrict__ Lbuf,
               float* __restrict__ dp, const int* __restrict__ info) {
  const int bid = blockIdx.x, tid = threadIdx.x;
  const float* LT = Lbuf + (size_t)bid * 2 * n * n + (size_t)n * n;
  float* xo = dp + (size_t)bid * n;
  __shared__ float pan[NB * PST];
  __shared__ float yv[NB];
  backward_subst<true>(LT, xo, n, pan, yv, tid);
  if (info[bid]) poison_row(xo, n, tid);
}
