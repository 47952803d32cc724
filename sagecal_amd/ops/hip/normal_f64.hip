// Float64 Gauss-Newton normal matrices of the influence map for gfx950
// (MI355X): JtJ [Mt, 8N, 8N] of every chunk of every cluster in two
// launches, from complex64 coherencies and solutions, with every product
// and every sum in float64. It is what reference.jtj_jtr assembles, in the
// parameter order of reference.vecR, without the data: JtJ does not depend
// on x.
//
// Closed form. With (p, q) = pairs[b], G = C J_q^H and K = J_p C (the G1 and
// K of solvers/diagnostics.py, from lev_products of leverage.hip), the 16x16
// Gram of [D1 D2] of one row has three blocks,
//   (p, p) = D1^T D1 = I2 (x) realify(Q1),  Q1[a][b] = sum_k conj(G[a][k]) G[b][k]
//   (q, q) = D2^T D2 = I2 (x) realify(Q2),  Q2[a][b] = sum_k K[k][a] conj(K[k][b])
//   (p, q) = D1^T D2, entry (2r + s, 2c + u) of the 2x2 pattern
//            [[Re x, Im x], [Im x, -Re x]] of x[r][c] = conj(G[j][k]) K[i][b],
//            r = 2i + j, c = 2k + b,
// and (q, p) its transpose. Q1 and Q2 are Hermitian 2x2, four reals each
// (q00, q11, Re q01, Im q01), and x is 16 complex numbers: NRM_NV = 40
// distinct float64 values per (pair, chunk), kept in registers across the
// timeslots of a piece. Everything else of the Gram is a copy, a sign or 0.
//
// Multiply-adds at the default shape (64 stations, 960 timeslots, 10
// clusters: 19,353,600 rows). (a) This closed form: 64 for G and K, 32 for
// Q1 and Q2, 64 for x and 40 to add them with the row's weight, 200 a row,
// 3.9e9 in all, 0.1 ms of the vector unit's float64 rate. (b) The matrix
// unit: the 16x16 Gram of one pair over K = 8 rows a timeslot is one
// v_mfma_f64_16x16x4_f64 accumulator tile, 16 * 16 * 8 = 2048 multiply-adds
// a row, 4.0e10 in all, at twice the rate of the vector unit five times the
// time of (a) and above the 0.17 ms the 619 MB of coherencies need; and the
// operands [D1 D2], 8x16 float64 a row, would have to be built in LDS from
// the same G and K first. 3/4 of its products multiply structural zeros and
// most of the rest repeat. (a) was built: it is bound by the coherency
// reads, (b) would be bound by arithmetic.
//
// k_normal_accum, grid (tiles of 64 pairs, pieces). A piece (ci, c, t0, t1)
// is a run of timeslots of cluster ci in chunk c, cut at
// hip_host.NORMAL_TSPLIT = 64 by the host. Lane = pair, so for one timeslot
// the coherency reads of a wave are 64 x 32 contiguous bytes; wave w of the
// four takes timeslots t0 + w, t0 + w + 4, ..., loads the next coherency
// before it works on the present one, and keeps J_p, J_q and the 40 sums in
// registers. The four waves then add up through red[40][65] in LDS (20,800
// bytes) in the fixed order ((w3 + w2) + w1) + w0, and the workgroup writes
// the tile's 64 x 40 sums, contiguous in part [E, Nbase, 40], with all 256
// threads; the row of 65 doubles keeps that transposing read off one bank.
// A pair with a negative entry reads no J and no coherency and stores zeros.
//
// k_normal_expand, grid (tile pairs I <= J of 8 x 8 stations, chunks),
// writes every entry of the output once: tile (I, J), 64 x 64 doubles, is
// built in LDS as tile[64][65] (33,280 bytes) and stored by rows of 512
// contiguous bytes, and for I < J stored again transposed, read down the
// columns of the same LDS tile, as tile (J, I); inside a diagonal tile the
// thread that builds block (s1, s2), s1 < s2, stores its values at the
// mirrored place too. So JtJ == JtJ^T to the bit, both halves from the same
// values. Four threads serve a block, one per row r of x: they add the
// pieces of the chunk in piece order (hip_host._lbfgs_extents sorts them by
// chunk, then cluster, then time) from 64 contiguous bytes per piece.
// pidx [N, N] names the pair of a block and which way round it is stored;
// a block without a pair is zero. Diagonal blocks are sums over the
// station's partners: in a diagonal tile 32 threads serve a station, thread
// (value, g) adds entries g, g + 8, ... of the station's list (sta_off,
// sta_ent of hip_host._lbfgs_stations, sorted by pair) and the eight groups
// are added in order 0..7 through dred in LDS (2 KB). No atomics, no
// float32, every order fixed; a chunk reads only its own pieces, so it does
// not depend on the batch.
//
// Compiler report for gfx950 (-Rpass-analysis=kernel-resource-usage):
//   k_normal_accum:  VGPRs 180, AGPRs 0, SGPRs 31, scratch 0 bytes/lane, no
//     spills, no dynamic stack, LDS 20,800 bytes, occupancy 2 waves/SIMD
//     (80 VGPRs are the sums, 32 the two solutions)
//   k_normal_expand: VGPRs 40, AGPRs 0, SGPRs 42, scratch 0 bytes/lane, no
//     spills, no dynamic stack, LDS 35,328 bytes, occupancy 4 waves/SIMD,
//     which is what LDS allows (four workgroups of four waves in 160 KB)
// Measured at the default shape: 0.322 ms for both, 3.6 TB/s over the 1.16
// GB they must move (profiles/normal_f64.json).
#include "common.h"

#define NRM_NW (NORMAL_F64_TB / WAVE)
#define NRM_NV NORMAL_F64_NV
static_assert(NRM_NV == 40, "Q1, Q2 and x");
#define NRM_LD 65                   // doubles per row of red and tile
static_assert(NORMAL_F64_TB == 256 && NRM_NW == 4,
              "k_normal_expand maps 256 threads to 64 blocks x 4 rows");

// one row's 40 values, times w, added to acc: Q1 at 0, Q2 at 4, x at 8
__device__ __forceinline__ void nrm_row(
    const double (&gr)[4], const double (&gi)[4], const double (&kr)[4],
    const double (&ki)[4], double w, double (&acc)[NRM_NV]) {
  acc[0] += w * (gr[0] * gr[0] + gi[0] * gi[0] + gr[1] * gr[1] + gi[1] * gi[1]);
  acc[1] += w * (gr[2] * gr[2] + gi[2] * gi[2] + gr[3] * gr[3] + gi[3] * gi[3]);
  acc[2] += w * (gr[0] * gr[2] + gi[0] * gi[2] + gr[1] * gr[3] + gi[1] * gi[3]);
  acc[3] += w * (gr[0] * gi[2] - gi[0] * gr[2] + gr[1] * gi[3] - gi[1] * gr[3]);
  acc[4] += w * (kr[0] * kr[0] + ki[0] * ki[0] + kr[2] * kr[2] + ki[2] * ki[2]);
  acc[5] += w * (kr[1] * kr[1] + ki[1] * ki[1] + kr[3] * kr[3] + ki[3] * ki[3]);
  acc[6] += w * (kr[0] * kr[1] + ki[0] * ki[1] + kr[2] * kr[3] + ki[2] * ki[3]);
  acc[7] += w * (ki[0] * kr[1] - kr[0] * ki[1] + ki[2] * kr[3] - kr[2] * ki[3]);
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      // conj(G[j][k]) K[i][b], r = 2i + j, c = 2k + b
      const int g = (r & 1) * 2 + (c >> 1), k = (r >> 1) * 2 + (c & 1);
      acc[8 + (r * 4 + c) * 2] += w * (gr[g] * kr[k] + gi[g] * ki[k]);
      acc[9 + (r * 4 + c) * 2] += w * (gr[g] * ki[k] - gi[g] * kr[k]);
    }
}

extern "C" __global__ void __launch_bounds__(NORMAL_F64_TB)
k_normal_accum(NormalF64Args a, double* __restrict__ part) {
  __shared__ double red[NRM_NV * NRM_LD];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int b0 = blockIdx.x * WAVE, b = b0 + lane;
  const int4 pc = reinterpret_cast<const int4*>(a.pieces)[blockIdx.y];
  const int ci = pc.x, c = pc.y, t0 = pc.z, t1 = pc.w;
  const size_t R = (size_t)a.T * a.Nbase;

  double acc[NRM_NV];
#pragma unroll
  for (int v = 0; v < NRM_NV; ++v) acc[v] = 0.0;
  int p = -1, q = -1;
  if (b < a.Nbase) { p = a.pairs[2 * b]; q = a.pairs[2 * b + 1]; }
  if (p >= 0 && q >= 0 && t0 + wave < t1) {
    double pr[4], pi[4], qr[4], qi[4];
    lev_load4(a.J + ((size_t)c * a.N + p) * 4, pr, pi);
    lev_load4(a.J + ((size_t)c * a.N + q) * 4, qr, qi);
    const float4* coh =
        reinterpret_cast<const float4*>(a.cohs + ((size_t)ci * R + b) * 4);
    const size_t step = (size_t)a.Nbase * 2;        // float4 per timeslot
    int t = t0 + wave;
    float4 n0 = coh[t * step], n1 = coh[t * step + 1];
    for (; t < t1; t += NRM_NW) {
      const float4 c0 = n0, c1 = n1;
      if (t + NRM_NW < t1) {
        n0 = coh[(t + NRM_NW) * step];
        n1 = coh[(t + NRM_NW) * step + 1];
      }
      const double cr[4] = {c0.x, c0.z, c1.x, c1.z};
      const double cim[4] = {c0.y, c0.w, c1.y, c1.w};
      double gr[4], gi[4], kr[4], ki[4];
      lev_products(cr, cim, pr, pi, qr, qi, gr, gi, kr, ki);
      const double w =
          a.wts != nullptr ? (double)a.wts[(size_t)t * a.Nbase + b] : 1.0;
      nrm_row(gr, gi, kr, ki, w, acc);
    }
  }

  // ((w3 + w2) + w1) + w0, a lane's own column of red
#pragma unroll
  for (int w = NRM_NW - 1; w >= 0; --w) {
    if (wave == w) {
#pragma unroll
      for (int v = 0; v < NRM_NV; ++v)
        red[v * NRM_LD + lane] =
            w == NRM_NW - 1 ? acc[v] : red[v * NRM_LD + lane] + acc[v];
    }
    __syncthreads();
  }
  const int nb = min(WAVE, a.Nbase - b0);
  double* dst = part + ((size_t)blockIdx.y * a.Nbase + b0) * NRM_NV;
  for (int e = tid; e < nb * NRM_NV; e += NORMAL_F64_TB)
    dst[e] = red[(e % NRM_NV) * NRM_LD + e / NRM_NV];
}

extern "C" __global__ void __launch_bounds__(NORMAL_F64_TB)
k_normal_expand(NormalF64Args a, const double* __restrict__ part,
                double* __restrict__ out) {
  __shared__ double tile[64 * NRM_LD];
  __shared__ double dred[8 * 4 * 8];
  const int tid = threadIdx.x, N = a.N, c = blockIdx.y;
  const int nt = (N + 7) / 8;
  int I = 0, rem = blockIdx.x;
  while (rem >= nt - I) { rem -= nt - I; ++I; }
  const int J = I + rem;
  const bool diag_tile = I == J;
  const int e0 = a.piece_off[c], e1 = a.piece_off[c + 1];
  const size_t pstep = (size_t)a.Nbase * NRM_NV;

  if (diag_tile) {
    // the four values of station s, partners g, g + 8, ... of its list
    const int st = tid >> 5, val = tid & 3, g = (tid >> 2) & 7;
    const int s = I * 8 + st;
    double sum = 0.0;
    if (s < N)
      for (int k = a.sta_off[s] + g; k < a.sta_off[s + 1]; k += 8) {
        const int ent = a.sta_ent[k];
        const double* src =
            part + (size_t)(ent >> 1) * NRM_NV + (ent & 1) * 4 + val;
        for (int e = e0; e < e1; ++e) sum += src[e * pstep];
      }
    dred[(st * 4 + val) * 8 + g] = sum;
    __syncthreads();
    if (g == 0) {
      double total = 0.0;
#pragma unroll
      for (int k = 0; k < 8; ++k) total += dred[(st * 4 + val) * 8 + k];
      dred[(st * 4 + val) * 8] = total;
    }
    __syncthreads();
  }

  // block (s1, s2) of the tile, thread `sub` rows 2 sub and 2 sub + 1
  const int blk = tid >> 2, sub = tid & 3, s1l = blk >> 3, s2l = blk & 7;
  const int s1 = I * 8 + s1l, s2 = J * 8 + s2l;
  if (!diag_tile || s1l < s2l) {
    const int code = s1 < N && s2 < N ? a.pidx[(size_t)s1 * N + s2] : -1;
    double xr[4] = {0.0, 0.0, 0.0, 0.0}, xi[4] = {0.0, 0.0, 0.0, 0.0};
    if (code >= 0) {
      const double* src = part + (size_t)(code >> 1) * NRM_NV + 8 + sub * 8;
      for (int e = e0; e < e1; ++e) {
        const double2* x = reinterpret_cast<const double2*>(src + e * pstep);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double2 d = x[k];
          xr[k] += d.x; xi[k] += d.y;
        }
      }
    }
    // stored as (s2, s1): the block at (s1, s2) is the transpose
    const bool rev = code >= 0 && (code & 1);
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r8 = 2 * sub + (e >> 1), c8 = 2 * k + (e & 1);
        const double v = e == 0 ? xr[k] : e == 3 ? -xr[k] : xi[k];
        const int row = s1l * 8 + (rev ? c8 : r8);
        const int col = s2l * 8 + (rev ? r8 : c8);
        tile[row * NRM_LD + col] = v;
        if (diag_tile) tile[col * NRM_LD + row] = v;
      }
  } else if (s1l == s2l) {
    // I2 (x) realify(Q), rows 2 sub and 2 sub + 1
    const double q00 = dred[(s1l * 4 + 0) * 8], q11 = dred[(s1l * 4 + 1) * 8];
    const double re = dred[(s1l * 4 + 2) * 8], im = dred[(s1l * 4 + 3) * 8];
    const bool lo = (sub & 1) == 0;               // rows 0, 1 or 2, 3 of R4
    const double r0[4] = {lo ? q00 : re, lo ? 0.0 : im,
                          lo ? re : q11, lo ? -im : 0.0};
    const double r1[4] = {lo ? 0.0 : -im, lo ? q00 : re,
                          lo ? im : 0.0, lo ? re : q11};
    const int half = sub >> 1;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool in = (j >> 2) == half;
      tile[(s1l * 8 + 2 * sub) * NRM_LD + s1l * 8 + j] = in ? r0[j & 3] : 0.0;
      tile[(s1l * 8 + 2 * sub + 1) * NRM_LD + s1l * 8 + j] =
          in ? r1[j & 3] : 0.0;
    }
  }
  __syncthreads();

  const int lane = tid & (WAVE - 1), wave = tid / WAVE;
  const size_t ld = (size_t)8 * N;
  double* O = out + (size_t)c * ld * ld;
  for (int r = wave; r < 64; r += NRM_NW) {
    const size_t row = (size_t)I * 64 + r, col = (size_t)J * 64 + lane;
    if (row < ld && col < ld) O[row * ld + col] = tile[r * NRM_LD + lane];
  }
  if (!diag_tile)
    for (int r = wave; r < 64; r += NRM_NW) {
      const size_t row = (size_t)J * 64 + r, col = (size_t)I * 64 + lane;
      if (row < ld && col < ld) O[row * ld + col] = tile[lane * NRM_LD + r];
    }
}
