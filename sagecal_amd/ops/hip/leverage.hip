// Influence-map leverage for gfx950 (MI355X): per visibility row and
// cluster, what solvers/diagnostics.leverage computes from a per-row gather
// of H^-1 [B, 8N, 8N], in ONE launch for all clusters and with every 8x8
// block of H^-1 read once per (pair, cluster, piece of timeslots).
//
// Closed form. With G1 = C J_q^H, K = J_p C (float64, from complex64 loads),
// M = realify(G1^T) and A = antirealify(K), both 4x4, the design blocks are
// D1 = diag(M, M) and D2 = P diag(A, A) with P the row permutation
// (0,1,4,5,2,3,6,7), and
//   lev = tr(D1 Hpp D1^T) + tr(D2 Hqq D2^T) + 2 tr(D1 Hpq D2^T)
//       = <M^T M, Hpp[0:4,0:4] + Hpp[4:8,4:8]>
//       + <A^T A, Hqq[0:4,0:4] + Hqq[4:8,4:8]>          (P^T P = I)
//       + 2 sum over rows i of Hpq, i = 4 a + i', of
//             sum_r M[r][i'] w[r],  w[0] = A[2a] . Hpq[i][0:4],
//             w[1] = A[2a+1] . Hpq[i][0:4], w[2] = A[2a] . Hpq[i][4:8],
//             w[3] = A[2a+1] . Hpq[i][4:8]
// (row i of D1^T D2 Hpq^T: column i of D1 has the four entries M[.][i'], and
// the four rows of D2 they meet hold rows 2a, 2a+1 of A in columns 0:4 or
// 4:8). M^T M and A^T A are symmetric, so of the two summed diagonal
// sub-blocks only s[i][j] = h[i][j] + h[j][i] (i < j) and h[i][i] enter: 10
// values for Hpp, 10 for Hqq and the 64 of Hpq, LEV_NV = 84 doubles per
// (pair, chunk). H^-1 is not assumed symmetric: both triangles are read and
// summed. Per row that is 64 products for G1 and K, 100 for the two Grams
// against Hpp and Hqq and 160 for the cross term. The cross term goes row by
// row of Hpq and not through X = D1^T D2 (128 + 64 products): the entries of
// M and A repeat, the compiler merges the equal products of X and keeps
// them, and the kernel then needs 256 VGPRs.
//
// Work split. The 84 doubles depend on (cluster, chunk, pair), not on the
// timeslot. grid = (tiles of 64 pairs, pieces); a piece (ci, c, t0, t1) is a
// run of timeslots of cluster ci with one chunk id c, cut at
// hip_host.LEVERAGE_TSPLIT = 64 by the host, so that a long chunk still
// spreads over the card while the staging below is paid once per 64 rows of
// a pair. The workgroup of LEVERAGE_TB = 256 threads first stages the 84
// doubles of its 64 pairs in LDS as hs[84][65]: for the Hpq part a wave reads one
// pair's 8x8 block, lane = entry, so a load instruction covers eight 64-byte
// row segments; the row of 65 (not 64) doubles spreads those stores, which
// go down a column, over the banks. After one barrier wave w takes the
// timeslots t0 + w, t0 + w + 4, ... with lane = pair: for a fixed t the coh
// reads (32 bytes per lane) and the lev stores are contiguous along b, and
// lane b reads its own column hs[k][b] without bank conflicts. J_p and J_q
// are loaded once per lane and kept in registers as doubles; the 84 doubles
// are not (168 VGPRs), they come from LDS for every row.
//
// A pair with a negative entry reads no H^-1 and no J, and its rows get 0.
// Every row is written by one lane and nothing is accumulated across lanes:
// no atomics, and two launches agree bit for bit.
//
// MFMA does not fit: the contraction pairs 84 per-row weights with 84
// per-pair values, a dot product per lane with no operand shared between
// rows of different pairs.
//
// Compiler report for gfx950 (-Rpass-analysis=kernel-resource-usage),
// k_leverage: VGPRs 136, AGPRs 0, SGPRs 43, scratch 0 bytes/lane, no spills,
// no dynamic stack, static LDS 43,680 bytes, occupancy 3 waves/SIMD, which
// is also what LDS allows (three workgroups of four waves in 160 KB). The
// scheduling barriers in lev_row are what keeps it there: without them the
// compiler moves all 84 LDS reads to the top of the row and reports 256
// VGPRs and 1 wave/SIMD.
#include "common.h"

#define LEV_NW (LEVERAGE_TB / WAVE)
#define LEV_NV 84
#define LEV_LD 65                   // doubles per row of hs
static_assert(LEVERAGE_TB % WAVE == 0, "whole waves");

// C J_q^H and J_p C in float64; 2x2 row-major, re and im apart
__device__ __forceinline__ void lev_products(
    const double (&cr)[4], const double (&ci)[4], const double (&pr)[4],
    const double (&pi)[4], const double (&qr)[4], const double (&qi)[4],
    double (&gr)[4], double (&gi)[4], double (&kr)[4], double (&ki)[4]) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      double xr = 0.0, xi = 0.0, yr = 0.0, yi = 0.0;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        // C[a][k] conj(Jq[b][k])
        xr += cr[a * 2 + k] * qr[b * 2 + k] + ci[a * 2 + k] * qi[b * 2 + k];
        xi += ci[a * 2 + k] * qr[b * 2 + k] - cr[a * 2 + k] * qi[b * 2 + k];
        // Jp[a][k] C[k][b]
        yr += pr[a * 2 + k] * cr[k * 2 + b] - pi[a * 2 + k] * ci[k * 2 + b];
        yi += pr[a * 2 + k] * ci[k * 2 + b] + pi[a * 2 + k] * cr[k * 2 + b];
      }
      gr[a * 2 + b] = xr; gi[a * 2 + b] = xi;
      kr[a * 2 + b] = yr; ki[a * 2 + b] = yi;
    }
}

// the leverage of one row from its G1 and K and column `col` of hs
__device__ __forceinline__ double lev_row(
    const double (&gr)[4], const double (&gi)[4], const double (&kr)[4],
    const double (&ki)[4], const double* col) {
  double M[4][4], A[4][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      // realify(G1^T): entry (a, b) is G1[b][a]
      M[2 * a][2 * b] = gr[b * 2 + a];
      M[2 * a][2 * b + 1] = -gi[b * 2 + a];
      M[2 * a + 1][2 * b] = gi[b * 2 + a];
      M[2 * a + 1][2 * b + 1] = gr[b * 2 + a];
      // antirealify(K)
      A[2 * a][2 * b] = kr[a * 2 + b];
      A[2 * a][2 * b + 1] = ki[a * 2 + b];
      A[2 * a + 1][2 * b] = ki[a * 2 + b];
      A[2 * a + 1][2 * b + 1] = -kr[a * 2 + b];
    }
  double diag = 0.0, cross = 0.0;
  int k = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i; j < 4; ++j, ++k) {
      const double s = M[0][i] * M[0][j] + M[1][i] * M[1][j] +
                       M[2][i] * M[2][j] + M[3][i] * M[3][j];
      const double u = A[0][i] * A[0][j] + A[1][i] * A[1][j] +
                       A[2][i] * A[2][j] + A[3][i] * A[3][j];
      diag += s * col[k * LEV_LD] + u * col[(10 + k) * LEV_LD];
    }
  const double* x = col + 20 * LEV_LD;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    // keeps the LDS reads of one row of Hpq together: hoisted to the top,
    // the 84 values would sit in registers after all
    __builtin_amdgcn_sched_barrier(0);
    const int a0 = i < 4 ? 0 : 2;
    double w[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double h0 = x[(i * 8 + j) * LEV_LD];
      const double h1 = x[(i * 8 + 4 + j) * LEV_LD];
      w[0] += A[a0][j] * h0;
      w[1] += A[a0 + 1][j] * h0;
      w[2] += A[a0][j] * h1;
      w[3] += A[a0 + 1][j] * h1;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) cross += M[r][i & 3] * w[r];
  }
  return diag + 2.0 * cross;
}

// one station's 2x2 Jones, widened
__device__ __forceinline__ void lev_load4(const cf* __restrict__ m,
                                          double (&re)[4], double (&im)[4]) {
  const float4 a = reinterpret_cast<const float4*>(m)[0];
  const float4 b = reinterpret_cast<const float4*>(m)[1];
  re[0] = a.x; im[0] = a.y; re[1] = a.z; im[1] = a.w;
  re[2] = b.x; im[2] = b.y; re[3] = b.z; im[3] = b.w;
}

__device__ __forceinline__ void leverage_body(
    const cf* __restrict__ cohs, const cf* __restrict__ J,
    const double* __restrict__ Hinv, const double* __restrict__ wts,
    const int* __restrict__ pairs, const int* __restrict__ pieces, int Nbase,
    int N, long long R, double* __restrict__ lev) {
  __shared__ double hs[LEV_NV * LEV_LD];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int b0 = blockIdx.x * WAVE;
  const int4 pc = reinterpret_cast<const int4*>(pieces)[blockIdx.y];
  const int ci = pc.x, c = pc.y, t0 = pc.z, t1 = pc.w;
  const size_t ld = (size_t)8 * N;
  const double* H = Hinv + (size_t)c * ld * ld;

  // Hpq: a wave per pair and pass, lane = entry (i, j) of the 8x8 block
  for (int e = tid; e < WAVE * 64; e += LEVERAGE_TB) {
    const int pl = e >> 6, i = (e >> 3) & 7, j = e & 7, b = b0 + pl;
    if (b >= Nbase) continue;
    const int p = pairs[2 * b], q = pairs[2 * b + 1];
    if (p < 0 || q < 0) continue;
    hs[(20 + i * 8 + j) * LEV_LD + pl] =
        H[((size_t)8 * p + i) * ld + (size_t)8 * q + j];
  }
  // the summed diagonal 4x4 sub-blocks of Hpp and Hqq, upper triangle
  for (int e = tid; e < WAVE * 20; e += LEVERAGE_TB) {
    const int pl = e / 20, r = e % 20, side = r / 10, k = r % 10, b = b0 + pl;
    if (b >= Nbase) continue;
    const int p = pairs[2 * b], q = pairs[2 * b + 1];
    if (p < 0 || q < 0) continue;
    const int i = k < 4 ? 0 : k < 7 ? 1 : k < 9 ? 2 : 3;
    const int j = k - (i == 0 ? 0 : i == 1 ? 3 : i == 2 ? 5 : 6);
    const size_t s8 = (size_t)8 * (side ? q : p);
    const double* D = H + s8 * ld + s8;
    double v = D[i * ld + j] + D[(4 + i) * ld + 4 + j];
    if (i != j) v += D[j * ld + i] + D[(4 + j) * ld + 4 + i];
    hs[(side * 10 + k) * LEV_LD + pl] = v;
  }
  __syncthreads();

  const int b = b0 + lane;
  if (b >= Nbase) return;
  const int p = pairs[2 * b], q = pairs[2 * b + 1];
  double* out = lev + (size_t)ci * R + b;
  if (p < 0 || q < 0) {
    for (int t = t0 + wave; t < t1; t += LEV_NW)
      out[(size_t)t * Nbase] = 0.0;
    return;
  }
  double pr[4], pi[4], qr[4], qi[4];
  lev_load4(J + ((size_t)c * N + p) * 4, pr, pi);
  lev_load4(J + ((size_t)c * N + q) * 4, qr, qi);
  const cf* coh = cohs + ((size_t)ci * R + b) * 4;
  for (int t = t0 + wave; t < t1; t += LEV_NW) {
    const size_t r = (size_t)t * Nbase;
    double cr[4], cim[4], gr[4], gi[4], kr[4], ki[4];
    lev_load4(coh + r * 4, cr, cim);
    lev_products(cr, cim, pr, pi, qr, qi, gr, gi, kr, ki);
    double v = lev_row(gr, gi, kr, ki, hs + lane);
    if (wts != nullptr) v *= wts[r + b];
    out[r] = v;
  }
}

extern "C" __global__ void __launch_bounds__(LEVERAGE_TB)
k_leverage(LeverageArgs a, double* lev) {
  leverage_body(a.cohs, a.J, a.Hinv, a.wts, a.pairs, a.pieces, a.Nbase, a.N,
                (long long)a.T * a.Nbase, lev);
}
