// Batched inverse of damped symmetric positive definite matrices for gfx950
// (MI355X), float64 throughout:
//   X = (A + mu I)^-1   per matrix, A [Mt, n, n] float32 or float64,
//   8 <= n <= SPD_INVERSE_MAXN, n a multiple of 8 (n = 8 N of the influence
// map), the float64 inverse that k_leverage (leverage.hip) consumes.
//
// Closed form. A + mu I = L L^T (right-looking blocked Cholesky), M = L^-1
// (blocked triangular inverse), X = M^T M. With U = M^T = L^-T, upper
// triangular, X = U U^T. All blocks are SPD_NB = 32 square; block (I, J) of a
// matrix is rows 32 I.., columns 32 J... Every rank-k update is
//   C[i][j] += sum_k P[i][k] Q[j][k]                                   (NT)
// on v_mfma_f64_16x16x4_f64 with P and Q row-major 32 x 32 blocks, which is
// why U and not M is what gets stored: the three products
//   trailing update   W[I][J] -= L[I][k] L[J][k]^T
//   inverse of L      S = sum_{K=j}^{I-1} U[j][K] L[I][K]^T,
//                     U[j][I] = -S M_II^T        (from L_II M_Ij = -sum ...)
//   final product     X[I][J] = sum_{K>=I} U[I][K] U[J][K]^T
// and the panel solve L[I][k] = W[I][k] M_kk^T all have that shape, with
// both operands read along rows of the stored matrix.
//
// Storage. The scratch W [Mt, n, n] holds L below the diagonal blocks (the
// trailing matrix before that) and U above them: the inverse is written into
// the free triangle, so no kernel overwrites what another workgroup of the
// same launch reads. The diagonal blocks of W keep the updated A_kk; their
// factor is never stored, only its inverse M_kk and U_kk = M_kk^T, in the
// scratch D [Mt, nt, 2, 32, 32]. The first panel and the first trailing
// update read A itself, widen it and add mu on the diagonal, so no float64
// copy of A + mu I is made beyond the scratch the factor needs anyway. Only
// the lower triangle of A is read.
//
// Kernel sequence, plain launches on one stream, nt = ceil(n / 32):
//   for kb = 0 .. nt-1:
//     k_spdinv_panel*  grid = Mt x max(1, row blocks below). Every workgroup
//                      factors the 32 x 32 diagonal block itself (wave 0, a
//                      row per lane in registers, columns broadcast by lane
//                      reads; sqrt and true division), inverts it (a column
//                      per lane, L broadcast from LDS), and multiplies its
//                      own row block by M_kk^T on the matrix unit.
//                      Factoring 32 x 32 redundantly costs
//                      a few microseconds and saves a launch per step and
//                      the round trip of L_kk through global memory; the
//                      first workgroup of a matrix stores M_kk and U_kk.
//     k_spdinv_syrk*   grid = Mt x lower tiles of the trailing matrix.
//   for I = 1 .. nt-1:
//     k_spdinv_trtri   grid = Mt x I: block column I of U, one workgroup per
//                      block (j, I), K loop over j..I-1.
//   k_spdinv_lauum     grid = Mt x nt(nt+1)/2: block (I, J), I >= J, of X,
//                      written to both triangles from the same registers
//                      (through LDS, so that both stores run along rows);
//                      on a diagonal block only i >= j is taken. A matrix
//                      with info set gets NaN instead.
// The *_f32 / *_f64 kernels are the kb = 0 variants that read A.
//
// Work split. One 256-thread workgroup per 32 x 32 output block, wave w the
// 16 x 16 fragment (w >> 1, w & 1), grid = batch x blocks. At 160 x 512 the
// largest launches have 19,200 (syrk) and 21,760 (lauum) workgroups; at
// 10 x 512, 1,200 and 1,360, still several per CU, where one workgroup per
// matrix would use 10 of 256 CUs. The steps of potrf and trtri are
// sequential per matrix (2 nt + nt launches), which is what bounds the small
// batch. A 32-wide block keeps the only scalar code, the diagonal factor
// and inverse, at 2 x 496 multiply-adds per lane.
//
// LDS. A staged block is [32][SPD_LD] doubles, SPD_LD = 34: 8,704 bytes;
// panel holds three (diagonal, row block, M_kk: 26,112 bytes), the others
// two (17,408 bytes). A fragment operand is P[i0 + (lane & 15)][kk + (lane
// >> 4)], K along the row, so the four K columns of a fragment are the
// lanes' quarter-waves. A double covers two 4-byte banks; with 64 banks a
// 64-bit read is served half a wave at a time, 16 rows x 2 K columns. The
// doubleword index is 34 i + kq = 2 i + kq (mod 32): for i = 0..15 and
// kq in {0, 1} or {2, 3} these are 32 different residues, so each half
// wave touches every bank pair once. The float32 strides of
// cholesky_blocked.hip (XB + 16 floats, K along the column) do not carry
// over: 34 floats would put rows 16 apart on one bank; here the stride has
// to be 2 (mod 32) in doublewords.
//
// Ragged n (24, 40, 136, ...): the last block has 8, 16 or 24 rows. Loads
// fill rows and columns beyond n with zeros, the diagonal block is
// completed by the identity, stores are masked. Nothing is padded on the
// host.
//
// One owner per element and fixed summation orders in every kernel, no
// float atomics: two calls agree bit for bit, and a matrix's result does
// not depend on the batch around it. A non-positive (or NaN) pivot sets
// info[matrix] (integer atomicOr, the contract of cholesky.hip), the factor
// goes on with pivot 1 and the matrix's X is NaN; the other matrices never
// see it. A is not written.
//
// Compiler report for gfx950 (-Rpass-analysis=kernel-resource-usage), all
// with scratch 0 bytes/lane, no VGPR or SGPR spills and no dynamic stack;
// the 8 AGPRs are the fragment's accumulator:
//   k_spdinv_panel, _f32, _f64   88 VGPRs, 8 AGPRs, 98 SGPRs, LDS 26,112 B,
//                                occupancy 5 waves/SIMD (the row in
//                                registers; L goes back through LDS before
//                                the inverse, which read by lane took 194
//                                VGPRs and spilled 50 SGPRs)
//   k_spdinv_syrk, _f32, _f64    18 VGPRs, 8 AGPRs, LDS 17,408 B, 8 waves/SIMD
//   k_spdinv_trtri               31 VGPRs, 8 AGPRs, LDS 17,408 B, 8 waves/SIMD
//   k_spdinv_lauum               28 VGPRs, 8 AGPRs, LDS 17,408 B, 8 waves/SIMD
// Measured on an MI355X (profiles/spd_inverse.json, float32 A): 160 x 512 in
// 1.84 ms and 10 x 512 in 0.64 ms, against 309.7 and 19.9 ms for
// torch.linalg.inv.
#include "common.h"

#define SPD_NB 32
#define SPD_LD 34                       // doubles per staged row
#define SPD_TB 256
#define SPD_BLK (SPD_NB * SPD_NB)
static_assert(SPD_TB == 4 * WAVE, "four 16 x 16 fragments per block");
static_assert(SPD_LD % 32 == 2, "bank layout of the fragment reads");

using spd_d4 = __attribute__((ext_vector_type(4))) double;

// rows 0..31 of a row-major block at src into dst [32][SPD_LD]; rows >= vr
// and columns >= vc (a multiple of 4) read as 0
template <typename T>
__device__ __forceinline__ void spd_stage(double* dst, const T* src,
                                          size_t ld, int vr, int vc,
                                          int tid) {
  const int r = tid >> 3, c = (tid & 7) << 2;
  double2 lo = {0.0, 0.0}, hi = {0.0, 0.0};
  if (r < vr && c < vc) {
    const T* p = src + (size_t)r * ld + c;
    if constexpr (sizeof(T) == 4) {
      const float4 f = *reinterpret_cast<const float4*>(p);
      lo = {(double)f.x, (double)f.y};
      hi = {(double)f.z, (double)f.w};
    } else {
      lo = reinterpret_cast<const double2*>(p)[0];
      hi = reinterpret_cast<const double2*>(p)[1];
    }
  }
  double2* d = reinterpret_cast<double2*>(dst + r * SPD_LD + c);
  d[0] = lo;
  d[1] = hi;
}

// acc += P[pr + i][0:32] . Q[qr + j][0:32] for one 16 x 16 fragment; lane
// (l15, l4) feeds row l15 and K column l4 of both operands and gets
// acc[reg] = C[4 reg + l4][l15] (the float64 instruction interleaves the
// rows over the quarter-waves, unlike mfma_f32_16x16x4f32 with 4 l4 + reg)
__device__ __forceinline__ spd_d4 spd_mma32(const double* P, int pr,
                                            const double* Q, int qr, int l15,
                                            int l4, spd_d4 acc) {
  const double* pa = P + (pr + l15) * SPD_LD + l4;
  const double* qb = Q + (qr + l15) * SPD_LD + l4;
#pragma unroll
  for (int kk = 0; kk < SPD_NB; kk += 4)
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[kk], qb[kk], acc, 0, 0, 0);
  return acc;
}

// Wave 0: the block in sd, completed by the identity beyond vr rows and
// shifted by `shift` on the diagonal, is factored in place (lane = row in
// registers, right looking, columns broadcast by lane reads). Returns
// whether a pivot was not positive.
__device__ __forceinline__ bool spd_factor(double* sd, int vr, double shift,
                                           int lane) {
  const int r = lane & 31;
  double a[SPD_NB];
#pragma unroll
  for (int c = 0; c < SPD_NB; ++c) {
    a[c] = sd[r * SPD_LD + c];
    if (c == r) a[c] = r < vr ? a[c] + shift : 1.0;
  }
  bool bad = false;
#pragma unroll
  for (int j = 0; j < SPD_NB; ++j) {
    double piv = __shfl(a[j], j, WAVE);
    if (!(piv > 0.0)) {
      bad = true;
      piv = 1.0;
    }
    const double s = sqrt(piv);
    a[j] = r == j ? s : a[j] / s;
    // rows above c carry values nobody reads
#pragma unroll
    for (int c = j + 1; c < SPD_NB; ++c)
      a[c] -= a[j] * __shfl(a[j], c, WAVE);
  }
  if (lane < SPD_NB) {
#pragma unroll
    for (int c = 0; c < SPD_NB; ++c) sd[r * SPD_LD + c] = a[c];
  }
  return bad;
}

// Wave 0: sm := L^-1 for the L in the lower triangle of sd, row-major with
// its zeros. Lane = column of L^-1, forward substitution down the rows; the
// entries of L are the same for every lane and come as LDS broadcasts.
__device__ __forceinline__ void spd_invert(const double* sd, double* sm,
                                           int lane) {
  const int r = lane & 31;
  double m[SPD_NB];
#pragma unroll
  for (int i = 0; i < SPD_NB; ++i) {
    double s = r == i ? 1.0 : 0.0;
#pragma unroll
    for (int q = 0; q < i; ++q) s -= sd[i * SPD_LD + q] * m[q];
    m[i] = r > i ? 0.0 : s / sd[i * SPD_LD + i];
  }
  if (lane < SPD_NB) {
#pragma unroll
    for (int i = 0; i < SPD_NB; ++i) sm[i * SPD_LD + lane] = m[i];
  }
}

// Step k of the factorisation: M_kk and U_kk to D, and row block s below the
// diagonal block := that block times M_kk^T. FIRST: the blocks come from A
// (widened, mu on the diagonal) and not from W.
template <typename TA, bool FIRST>
__device__ __forceinline__ void spd_panel_body(
    const TA* __restrict__ A, const double* __restrict__ mu, int mu_stride,
    double* __restrict__ W, double* __restrict__ D, int* __restrict__ info,
    int n, int k, int nb) {
  __shared__ __attribute__((aligned(16))) double sd[SPD_NB * SPD_LD];
  __shared__ __attribute__((aligned(16))) double ss[SPD_NB * SPD_LD];
  __shared__ __attribute__((aligned(16))) double sm[SPD_NB * SPD_LD];
  const int nbm = nb > 0 ? nb : 1;
  const int b = blockIdx.x / nbm, s = blockIdx.x % nbm;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int nt = (n + SPD_NB - 1) / SPD_NB;
  const size_t base = (size_t)b * n * n;
  const int r0 = k + SPD_NB + SPD_NB * s;
  const size_t od = base + (size_t)k * n + k, os = base + (size_t)r0 * n + k;
  if constexpr (FIRST) {
    spd_stage(sd, A + od, n, n - k, n - k, tid);
    if (nb > 0) spd_stage(ss, A + os, n, n - r0, n - k, tid);
  } else {
    spd_stage(sd, W + od, n, n - k, n - k, tid);
    if (nb > 0) spd_stage(ss, W + os, n, n - r0, n - k, tid);
  }
  __syncthreads();
  if (w == 0) {
    const double shift = FIRST ? mu[(size_t)b * mu_stride] : 0.0;
    const bool bad = spd_factor(sd, n - k, shift, lane);
    if (bad && lane == 0) atomicOr(&info[b], 1);
  }
  __syncthreads();
  if (w == 0) spd_invert(sd, sm, lane);
  __syncthreads();
  if (s == 0) {
    double* Dk = D + ((size_t)b * nt + k / SPD_NB) * 2 * SPD_BLK;
    for (int e = tid; e < SPD_BLK; e += SPD_TB) {
      const int i = e >> 5, j = e & 31;
      Dk[e] = sm[i * SPD_LD + j];
      Dk[SPD_BLK + e] = sm[j * SPD_LD + i];
    }
  }
  if (nb == 0) return;
  const int fi = (w >> 1) * 16, fj = (w & 1) * 16;
  const spd_d4 z = {0.0, 0.0, 0.0, 0.0};
  const spd_d4 acc = spd_mma32(ss, fi, sm, fj, l15, l4, z);
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int row = r0 + fi + reg * 4 + l4;
    if (row < n) W[base + (size_t)row * n + k + fj + l15] = acc[reg];
  }
}

// tile t of the lower triangle of the block grid that starts at block
// k / 32 + 1: W[I][J] -= L[I][k] L[J][k]^T
template <typename TA, bool FIRST>
__device__ __forceinline__ void spd_syrk_body(
    const TA* __restrict__ A, const double* __restrict__ mu, int mu_stride,
    double* __restrict__ W, int n, int k, int ntiles) {
  __shared__ __attribute__((aligned(16))) double sp[SPD_NB * SPD_LD];
  __shared__ __attribute__((aligned(16))) double sq[SPD_NB * SPD_LD];
  const int b = blockIdx.x / ntiles, t = blockIdx.x % ntiles;
  int I = (int)((sqrtf(8.0f * t + 1.0f) - 1.0f) * 0.5f + 1e-4f);
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  while (I * (I + 1) / 2 > t) --I;
  const int J = t - I * (I + 1) / 2;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  const int l15 = lane & 15, l4 = lane >> 4;
  const size_t base = (size_t)b * n * n;
  const int r0 = k + SPD_NB * (I + 1), c0 = k + SPD_NB * (J + 1);
  spd_stage(sp, W + base + (size_t)r0 * n + k, n, n - r0, n - k, tid);
  spd_stage(sq, W + base + (size_t)c0 * n + k, n, n - c0, n - k, tid);
  __syncthreads();
  const int fi = (w >> 1) * 16, fj = (w & 1) * 16;
  const spd_d4 z = {0.0, 0.0, 0.0, 0.0};
  const spd_d4 acc = spd_mma32(sp, fi, sq, fj, l15, l4, z);
  const int col = c0 + fj + l15;
  if (col >= n) return;
  const double shift = FIRST ? mu[(size_t)b * mu_stride] : 0.0;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int row = r0 + fi + reg * 4 + l4;
    if (row >= n) continue;
    const size_t o = base + (size_t)row * n + col;
    double c;
    if constexpr (FIRST)
      c = (double)A[o] + (row == col ? shift : 0.0);
    else
      c = W[o];
    W[o] = c - acc[reg];
  }
}

// block (j, I) of U, j < I, from block row I of L, the blocks (j, j..I-1)
// of U and M_II
__device__ __forceinline__ void spd_trtri_body(double* __restrict__ W,
                                               const double* __restrict__ D,
                                               int n, int I) {
  __shared__ __attribute__((aligned(16))) double sp[SPD_NB * SPD_LD];
  __shared__ __attribute__((aligned(16))) double sq[SPD_NB * SPD_LD];
  const int b = blockIdx.x / I, j = blockIdx.x % I;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int nt = (n + SPD_NB - 1) / SPD_NB;
  const size_t base = (size_t)b * n * n;
  const double* Db = D + (size_t)b * nt * 2 * SPD_BLK;
  const int rI = SPD_NB * I, rj = SPD_NB * j;
  const int fi = (w >> 1) * 16, fj = (w & 1) * 16;
  spd_d4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int K = j; K < I; ++K) {
    const int cK = SPD_NB * K;
    if (K == j)
      spd_stage(sp, Db + (size_t)j * 2 * SPD_BLK + SPD_BLK, SPD_NB, SPD_NB,
                SPD_NB, tid);
    else
      spd_stage(sp, W + base + (size_t)rj * n + cK, n, SPD_NB, SPD_NB, tid);
    spd_stage(sq, W + base + (size_t)rI * n + cK, n, n - rI, SPD_NB, tid);
    __syncthreads();
    acc = spd_mma32(sp, fi, sq, fj, l15, l4, acc);
    __syncthreads();
  }
  // S [c][b] back through LDS as the row operand of S M_II^T
#pragma unroll
  for (int reg = 0; reg < 4; ++reg)
    sp[(fi + reg * 4 + l4) * SPD_LD + fj + l15] = acc[reg];
  spd_stage(sq, Db + (size_t)I * 2 * SPD_BLK, SPD_NB, SPD_NB, SPD_NB, tid);
  __syncthreads();
  const spd_d4 z = {0.0, 0.0, 0.0, 0.0};
  const spd_d4 out = spd_mma32(sp, fi, sq, fj, l15, l4, z);
  const int col = rI + fj + l15;
  if (col >= n) return;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg)
    W[base + (size_t)(rj + fi + reg * 4 + l4) * n + col] = -out[reg];
}

// block (I, J), I >= J, of X = U U^T and its mirror image
__device__ __forceinline__ void spd_lauum_body(const double* __restrict__ W,
                                               const double* __restrict__ D,
                                               const int* __restrict__ info,
                                               int n, int ntiles,
                                               double* __restrict__ X) {
  __shared__ __attribute__((aligned(16))) double sp[SPD_NB * SPD_LD];
  __shared__ __attribute__((aligned(16))) double sq[SPD_NB * SPD_LD];
  const int b = blockIdx.x / ntiles, t = blockIdx.x % ntiles;
  int I = (int)((sqrtf(8.0f * t + 1.0f) - 1.0f) * 0.5f + 1e-4f);
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  while (I * (I + 1) / 2 > t) --I;
  const int J = t - I * (I + 1) / 2;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int nt = (n + SPD_NB - 1) / SPD_NB;
  const size_t base = (size_t)b * n * n;
  const double* Db = D + (size_t)b * nt * 2 * SPD_BLK;
  const int rI = SPD_NB * I, rJ = SPD_NB * J;
  const int fi = (w >> 1) * 16, fj = (w & 1) * 16;
  spd_d4 acc = {0.0, 0.0, 0.0, 0.0};
  if (info[b] == 0) {
    for (int K = I; K < nt; ++K) {
      const int cK = SPD_NB * K;
      const double* Uk = Db + (size_t)K * 2 * SPD_BLK + SPD_BLK;
      if (K == I)
        spd_stage(sp, Uk, SPD_NB, SPD_NB, SPD_NB, tid);
      else
        spd_stage(sp, W + base + (size_t)rI * n + cK, n, SPD_NB, n - cK, tid);
      if (K == J)
        spd_stage(sq, Uk, SPD_NB, SPD_NB, SPD_NB, tid);
      else
        spd_stage(sq, W + base + (size_t)rJ * n + cK, n, SPD_NB, n - cK, tid);
      __syncthreads();
      acc = spd_mma32(sp, fi, sq, fj, l15, l4, acc);
      __syncthreads();
    }
  } else {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    acc = {nan, nan, nan, nan};
  }
#pragma unroll
  for (int reg = 0; reg < 4; ++reg)
    sp[(fi + reg * 4 + l4) * SPD_LD + fj + l15] = acc[reg];
  __syncthreads();
  double* Xb = X + base;
  for (int e = tid; e < SPD_BLK; e += SPD_TB) {
    const int hi = e >> 5, lo = e & 31;
    // X[I-block row hi][J-block column lo]
    if (rI + hi < n && rJ + lo < n && (I != J || hi >= lo))
      Xb[(size_t)(rI + hi) * n + rJ + lo] = sp[hi * SPD_LD + lo];
    // its mirror image X[J-block row hi][I-block column lo]
    if (rJ + hi < n && rI + lo < n && (I != J || lo > hi))
      Xb[(size_t)(rJ + hi) * n + rI + lo] = sp[lo * SPD_LD + hi];
  }
}

#define SPD_FIRST_KERNELS(suffix, TA)                                        \
  extern "C" __global__ void __launch_bounds__(SPD_TB)                       \
  k_spdinv_panel##suffix(SpdInverseArgs a, int k, int nb) {                  \
    spd_panel_body<TA, true>(static_cast<const TA*>(a.A), a.mu,              \
                             a.mu_stride, a.W, a.D, a.info, a.n, k, nb);     \
  }                                                                          \
  extern "C" __global__ void __launch_bounds__(SPD_TB)                       \
  k_spdinv_syrk##suffix(SpdInverseArgs a, int k, int ntiles) {               \
    spd_syrk_body<TA, true>(static_cast<const TA*>(a.A), a.mu, a.mu_stride,  \
                            a.W, a.n, k, ntiles);                            \
  }
SPD_FIRST_KERNELS(_f32, float)
SPD_FIRST_KERNELS(_f64, double)
#undef SPD_FIRST_KERNELS

extern "C" __global__ void __launch_bounds__(SPD_TB)
k_spdinv_panel(SpdInverseArgs a, int k, int nb) {
  spd_panel_body<double, false>(nullptr, a.mu, a.mu_stride, a.W, a.D, a.info,
                                a.n, k, nb);
}

extern "C" __global__ void __launch_bounds__(SPD_TB)
k_spdinv_syrk(SpdInverseArgs a, int k, int ntiles) {
  spd_syrk_body<double, false>(nullptr, a.mu, a.mu_stride, a.W, a.n, k,
                               ntiles);
}

extern "C" __global__ void __launch_bounds__(SPD_TB)
k_spdinv_trtri(SpdInverseArgs a, int I) {
  spd_trtri_body(a.W, a.D, a.n, I);
}

extern "C" __global__ void __launch_bounds__(SPD_TB)
k_spdinv_lauum(SpdInverseArgs a, double* X) {
  const int nt = (a.n + SPD_NB - 1) / SPD_NB;
  spd_lauum_body(a.W, a.D, a.info, a.n, nt * (nt + 1) / 2, X);
}
