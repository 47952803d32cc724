// Diffuse-cluster predict with the spatial model applied, for gfx950
// (MI355X): what shapelet.recalculate_diffuse_coherencies computes on the
// host, per baseline row r = t*Nbase + b with (p, q) = pairs[b],
//   V_r = 2 pi sum_kl basis_kl(-u f, v f; g2) H_pq[k,l]
//         * exp(i phase) * |sinc(G fdelta / 2)|
//   H_pq = Z_p x (C x Z_q^H)        (Jones-valued Gauss-Hermite series products)
// with n1 = Gc + Gz - 1, n2 = Gz + n1 - 1, T1 [n1, Gc, Gz] and T2 [n2, Gz, n1]
// the 1-D product tensors (float64, built by the host's quadrature), modes
// indexed [n2][n1], 2x2 blocks row-major:
//   CZ_q[c,d] = sum_{a,b<Gc; e,f<Gz} T1[c,a,e] T1[d,b,f] C[a,b] Z_q[e,f]^H
//   H_pq[k,l] = sum_{a,b<Gz; c,d<n1} T2[k,a,c] T2[l,b,d] Z_p[a,b] CZ_q[c,d]
// All series products are float64 (the coefficients alternate in sign and
// cancel); the mode sum of the evaluation is float32 like k_shapelet_coh.
//
// Split of H_pq. Everything that depends on one station is done once per
// station, and that is more than CZ_q: with
//   P_p[k,c,b] = sum_a T2[k,a,c] Z_p[a,b]          (first axis,  station p)
//   R_q[c,l,b] = sum_d T2[l,b,d] CZ_q[c,d]         (second axis, station q)
// the pair is left with ONE contraction,
//   H_pq[k,l] = sum_{c<n1, b<Gz} P_p[k,c,b] R_q[c,l,b]      (2x2 products)
// a complex (2 n2) x (2 n1 Gz) x (2 n2) matrix product. The second axis is
// contracted with T2 before the pair product and not after it: P_p x CZ_q
// first would leave a [n2, Gz, n1] 2x2 intermediate per pair (237 KB at
// n2 = 32, Gz = 4, four times the LDS of a workgroup) and cost 9.1 instead
// of 7.6 MFLOP per pair.
//
// k_diffuse_station, grid (N, n1 + 1), 256 threads. Workgroup (s, c), c < n1,
// makes row c of CZ_s and from it the columns (c, ., .) of R_s, axis by axis
// through LDS, four barriers:
//   s1[e,b]  = sum_a T1[c,a,e] C[a,b]               Gz Gc blocks
//   s2[b,f]  = sum_e s1[e,b] Z_s[e,f]^H             Gc Gz blocks
//   cz[d]    = sum_{b,f} T1[d,b,f] s2[b,f]          n1 blocks
//   R[c,l,b] = sum_d T2[l,b,d] cz[d]                n2 Gz blocks
// s1 does not depend on the station; it is 4 Gc^2 Gz multiply-adds, less
// than a launch of its own and the trip through global memory would cost. A
// row per workgroup and not a station per workgroup: 64 workgroups would use
// a quarter of the card, and CZ_s whole (64 KB at n1 = 32) does not fit
// beside the rest. Workgroup (s, n1) makes P_s. Both are written in the form
// the pair kernel multiplies, real matrices with K along the row and zero
// padding to whole tiles, so that staging is a plain copy:
//   A[s][2k+i][kr]        kr = 2 ((c Gz + b) 2 + j) + part: Re, Im P[i][j]
//   B[s][4l+2m+ri][kr]    ri = 0: (Re R[j][m], -Im R[j][m])
//                         ri = 1: (Im R[j][m],  Re R[j][m])
// RA = 2 n2 and RB = 4 n2 rows rounded up to 16, Kp = 4 n1 Gz rounded up to
// 16: C = A B^T is then (Re, Im) of H_pq[k,l][i][m] at C[2k+i][4l+2m+ri].
//
// k_diffuse_pair, grid Nbase, 256 threads, one workgroup per pair.
// Stage 1: K in chunks of 16 through LDS, rows of DIF_LD = 18 doubles (18 i
// + kq takes 32 different residues mod 32 for 16 rows and two K columns, the
// rule of spd_inverse.hip). For n2 >= 8 the output has at least one full 16
// x 16 tile of rows and two of columns and goes to
// v_mfma_f64_16x16x4_f64: up to 4 x 8 tiles, wave w the tiles w, w + 4, ...
// (at n2 = 32 one tile row and all eight tile columns, the A fragment
// shared), 8 accumulators of 4 doubles. For n2 < 8 (at most 14 x 28 outputs)
// a padded tile would be mostly zeros and a thread takes two outputs with
// plain FMA from the same LDS chunks. H_pq then goes to LDS as float32, over
// the staging buffers, times 2 pi i^(k+l), the sign pattern of
// uv_mode_vectors; it is never written to global memory.
// Stage 2: lane = timeslot (t = lane, lane + 64, ...), wave w the rows
// k = w (mod 4) of the modes. Each lane runs the two normalised Hermite
// recurrences in registers as k_shapelet_coh does and reads H as broadcast
// float4. The four partial sums meet in LDS and wave 0 adds them in the
// order 0..3, applies the phase (float64 argument reduced mod 2 pi, float
// sincos) and the smearing (float64, guard 1e-12), and stores the row as two
// float4.
//
// A pair with a negative entry gets zeros. One owner per output, fixed
// summation orders, no atomics: two calls give the same bits.
//
// LDS: station 19,456 bytes; pair 32,768 (H; staging is 27,648 of it) +
// 8,192 (partial sums) + 256. DIFFUSE_MAX_N2 = 32 is where 2 n2 rows fill
// the four waves' tile rows and H fills its 32 KB.
//
// Compiler report for gfx950 (-Rpass-analysis=kernel-resource-usage), both
// with scratch 0 bytes/lane, no VGPR or SGPR spills and no dynamic stack:
//   k_diffuse_station  62 VGPRs, 0 AGPRs, 54 SGPRs, LDS 19,456 B, 8 waves/SIMD
//   k_diffuse_pair     96 VGPRs, 64 AGPRs (the 8 accumulators), 93 SGPRs,
//                      LDS 41,216 B, occupancy 3 waves/SIMD, which is also
//                      what LDS allows (three workgroups in 160 KB)
#include "common.h"

#define DIF_TB 256
#define DIF_NW (DIF_TB / WAVE)
#define DIF_KC 16
#define DIF_LD 18                       // doubles per staged row
#define DIF_MFMA_MIN_N2 8
static_assert(DIF_LD % 32 == 18 && DIF_LD >= DIF_KC, "bank layout");
static_assert(DIF_TB / 4 * 2 >= 4 * DIFFUSE_MAX_N2 &&
              DIF_NW * 16 >= 2 * DIFFUSE_MAX_N2, "staging and tile rows");

using dif_d4 = __attribute__((ext_vector_type(4))) double;

__device__ __forceinline__ void diffuse_station_body(
    const double2* __restrict__ Z, const double2* __restrict__ C,
    const double* __restrict__ T1, const double* __restrict__ T2,
    double* __restrict__ A, double* __restrict__ B, int Gz, int Gc) {
  __shared__ double2 zs[DIFFUSE_MAX_GZ * DIFFUSE_MAX_GZ * 4];
  __shared__ double2 s1[DIFFUSE_MAX_GZ * DIFFUSE_MAX_N2 * 4];
  __shared__ double2 s2[DIFFUSE_MAX_GZ * DIFFUSE_MAX_N2 * 4];
  __shared__ double2 cz[DIFFUSE_MAX_N2 * 4];
  const int n1 = Gc + Gz - 1, n2 = Gz + n1 - 1;
  const int RA = DIFFUSE_PAD16(2 * n2), RB = DIFFUSE_PAD16(4 * n2);
  const int Kr = 4 * n1 * Gz, Kp = DIFFUSE_PAD16(Kr);
  const int s = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  for (int e = tid; e < Gz * Gz * 4; e += DIF_TB)
    zs[e] = Z[(size_t)s * Gz * Gz * 4 + e];
  __syncthreads();

  if (c == n1) {
    // P_s with its padding, and the K padding of B
    double* As = A + (size_t)s * RA * Kp;
    const int kh = Kp / 2;
    for (int e = tid; e < RA * kh; e += DIF_TB) {
      const int row = e / kh, kc = e % kh;
      double2 val = {0.0, 0.0};
      if (row < 2 * n2 && 2 * kc < Kr) {
        const int k = row >> 1, i = row & 1, j = kc & 1;
        const int b = (kc >> 1) % Gz, cc = (kc >> 1) / Gz;
        for (int a = 0; a < Gz; ++a) {
          const double t = T2[(k * Gz + a) * n1 + cc];
          const double2 z = zs[(a * Gz + b) * 4 + i * 2 + j];
          val.x += t * z.x;
          val.y += t * z.y;
        }
      }
      *reinterpret_cast<double2*>(As + (size_t)row * Kp + 2 * kc) = val;
    }
    double* Bs = B + (size_t)s * RB * Kp;
    const int pad = Kp - Kr;
    for (int e = tid; e < RB * pad; e += DIF_TB)
      Bs[(size_t)(e / pad) * Kp + Kr + e % pad] = 0.0;
    return;
  }

  for (int e = tid; e < Gz * Gc * 4; e += DIF_TB) {
    const int ij = e & 3, b = (e >> 2) % Gc, cc = (e >> 2) / Gc;
    double2 acc = {0.0, 0.0};
    for (int a = 0; a < Gc; ++a) {
      const double t = T1[(c * Gc + a) * Gz + cc];
      const double2 x = C[(a * Gc + b) * 4 + ij];
      acc.x += t * x.x;
      acc.y += t * x.y;
    }
    s1[(cc * Gc + b) * 4 + ij] = acc;
  }
  __syncthreads();
  for (int e = tid; e < Gc * Gz * 4; e += DIF_TB) {
    const int i = (e >> 1) & 1, m = e & 1, d = (e >> 2) % Gz, b = (e >> 2) / Gz;
    double2 acc = {0.0, 0.0};
    for (int cc = 0; cc < Gz; ++cc)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        // s1[cc,b][i][j] conj(Z[cc,d][m][j])
        const double2 x = s1[(cc * Gc + b) * 4 + i * 2 + j];
        const double2 z = zs[(cc * Gz + d) * 4 + m * 2 + j];
        acc.x += x.x * z.x + x.y * z.y;
        acc.y += x.y * z.x - x.x * z.y;
      }
    s2[(b * Gz + d) * 4 + i * 2 + m] = acc;
  }
  __syncthreads();
  for (int e = tid; e < n1 * 4; e += DIF_TB) {
    const int im = e & 3, l = e >> 2;
    const double* t1 = T1 + (size_t)l * Gc * Gz;
    double2 acc = {0.0, 0.0};
    for (int bd = 0; bd < Gc * Gz; ++bd) {
      const double t = t1[bd];
      const double2 x = s2[bd * 4 + im];
      acc.x += t * x.x;
      acc.y += t * x.y;
    }
    cz[e] = acc;
  }
  __syncthreads();
  double* Bs = B + (size_t)s * RB * Kp;
  for (int e = tid; e < RB / 2 * Gz * 2; e += DIF_TB) {
    const int j = e & 1, b = (e >> 1) % Gz, lm = (e >> 1) / Gz;
    const int l = lm >> 1, m = lm & 1;
    double2 val = {0.0, 0.0};
    if (l < n2) {
      const double* t2 = T2 + (size_t)(l * Gz + b) * n1;
      for (int d = 0; d < n1; ++d) {
        const double t = t2[d];
        const double2 x = cz[d * 4 + j * 2 + m];
        val.x += t * x.x;
        val.y += t * x.y;
      }
    }
    double* o = Bs + (size_t)(2 * lm) * Kp + 2 * ((c * Gz + b) * 2 + j);
    *reinterpret_cast<double2*>(o) = double2{val.x, -val.y};
    *reinterpret_cast<double2*>(o + Kp) = double2{val.y, val.x};
  }
}

__device__ __forceinline__ void diffuse_pair_body(
    const double* __restrict__ u, const double* __restrict__ v,
    const double* __restrict__ w, const int* __restrict__ pairs,
    const double* __restrict__ A, const double* __restrict__ B, int T,
    int Nbase, int Gz, int Gc, double g2, double ll, double mm, double nn1,
    double freq, double fdelta2, float2* __restrict__ out) {
  // the staged chunks of A (64 rows) and B (128 rows), then H as float32
  __shared__ __attribute__((aligned(16)))
      double sm[DIFFUSE_MAX_N2 * DIFFUSE_MAX_N2 * 4];
  __shared__ __attribute__((aligned(16))) float red[DIF_NW * WAVE * 8];
  __shared__ float rec[2 * DIFFUSE_MAX_N2];
  static_assert(sizeof(sm) >= 6 * DIFFUSE_MAX_N2 * DIF_LD * sizeof(double),
                "staging fits under H");
  const int n1 = Gc + Gz - 1, n2 = Gz + n1 - 1;
  const int RA = DIFFUSE_PAD16(2 * n2), RB = DIFFUSE_PAD16(4 * n2);
  const int Kp = DIFFUSE_PAD16(4 * n1 * Gz);
  const int b = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & (WAVE - 1), wv = tid / WAVE;
  const int p = pairs[2 * b], q = pairs[2 * b + 1];
  if (p < 0 || q < 0) {
    const float4 z = {0.f, 0.f, 0.f, 0.f};
    for (int t = tid; t < T; t += DIF_TB) {
      float4* o = reinterpret_cast<float4*>(out + ((size_t)t * Nbase + b) * 4);
      o[0] = z;
      o[1] = z;
    }
    return;
  }

  // stage 1: C = A_p B_q^T
  double* sA = sm;
  double* sB = sm + 2 * DIFFUSE_MAX_N2 * DIF_LD;
  const double* Ap = A + (size_t)p * RA * Kp;
  const double* Bq = B + (size_t)q * RB * Kp;
  const bool mfma = n2 >= DIF_MFMA_MIN_N2;
  const int nA = RA / 16, ntile = nA * (RB / 16);
  const int l15 = lane & 15, l4 = lane >> 4;
  const int nc = 4 * n2, nout = 2 * n2 * nc;     // the plain route
  const int srow = tid >> 2, sseg = (tid & 3) * 4;
  dif_d4 acc[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) acc[s] = {0.0, 0.0, 0.0, 0.0};
  double f[2] = {0.0, 0.0};
  for (int kc = 0; kc < Kp; kc += DIF_KC) {
    if (srow < RA) {
      const double2* g = reinterpret_cast<const double2*>(
          Ap + (size_t)srow * Kp + kc + sseg);
      double2* d = reinterpret_cast<double2*>(sA + srow * DIF_LD + sseg);
      d[0] = g[0];
      d[1] = g[1];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int rb = srow + h * (DIF_TB / 4);
      if (rb < RB) {
        const double2* g = reinterpret_cast<const double2*>(
            Bq + (size_t)rb * Kp + kc + sseg);
        double2* d = reinterpret_cast<double2*>(sB + rb * DIF_LD + sseg);
        d[0] = g[0];
        d[1] = g[1];
      }
    }
    __syncthreads();
    if (mfma) {
#pragma unroll
      for (int kk = 0; kk < DIF_KC; kk += 4)
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const int t = wv + DIF_NW * s;
          if (t < ntile) {
            const int ti = t % nA, tj = t / nA;
            acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                sA[(ti * 16 + l15) * DIF_LD + kk + l4],
                sB[(tj * 16 + l15) * DIF_LD + kk + l4], acc[s], 0, 0, 0);
          }
        }
    } else {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int o = tid + h * DIF_TB;
        if (o < nout) {
          const double* pa = sA + (o / nc) * DIF_LD;
          const double* pb = sB + (o % nc) * DIF_LD;
#pragma unroll
          for (int kk = 0; kk < DIF_KC; ++kk) f[h] += pa[kk] * pb[kk];
        }
      }
    }
    __syncthreads();
  }

  // H[k,l][i][m] (re, im) = C[2k+i][4l+2m+ri], as float over the staging
  float* Hs = reinterpret_cast<float*>(sm);
  auto put = [&](int row, int col, double val) {
    const int k = row >> 1, l = col >> 2;
    if (k < n2 && l < n2)
      Hs[(k * n2 + l) * 8 + (row & 1) * 4 + (col & 3)] = (float)val;
  };
  if (mfma) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int t = wv + DIF_NW * s;
      if (t < ntile) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          put((t % nA) * 16 + 4 * reg + l4, (t / nA) * 16 + l15, acc[s][reg]);
      }
    }
  } else {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int o = tid + h * DIF_TB;
      if (o < nout) put(o / nc, o % nc, f[h]);
    }
  }
  if (tid < n2) {
    const double n = tid > 0 ? (double)tid : 1.0;
    rec[tid] = (float)sqrt(2.0 / n);
    rec[DIFFUSE_MAX_N2 + tid] = (float)sqrt((n - 1.0) / n);
  }
  __syncthreads();
  // times 2 pi i^(k+l): the sign and real/imaginary pattern of the basis
  for (int e = tid; e < n2 * n2 * 4; e += DIF_TB) {
    const int kl = e >> 2, rot = (kl / n2 + kl % n2) & 3;
    float2* hp = reinterpret_cast<float2*>(Hs) + e;
    const float2 c = *hp;
    const float tp = 6.283185307179586f;
    *hp = rot == 0 ? float2{tp * c.x, tp * c.y}
        : rot == 1 ? float2{-tp * c.y, tp * c.x}
        : rot == 2 ? float2{-tp * c.x, -tp * c.y}
                   : float2{tp * c.y, -tp * c.x};
  }
  __syncthreads();

  // stage 2: the mode sum, lane = timeslot, wave = rows k = wv (mod 4)
  const float* rec0 = rec;                     // sqrt(2/n)
  const float* rec1 = rec + DIFFUSE_MAX_N2;    // sqrt((n-1)/n)
  for (int t0 = 0; t0 < T; t0 += WAVE) {
    const int t = t0 + lane;
    const bool live = t < T;
    const size_t r = (size_t)(live ? t : 0) * Nbase + b;
    const double ur = u[r], vr = v[r];
    const float xu = (float)(-(ur * freq) * g2), xv = (float)(vr * freq * g2);
    const float pu0 = 0.70710678118654752f * expf(-0.5f * xu * xu);
    float a8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float pv1 = 0.f, pv = 0.70710678118654752f * expf(-0.5f * xv * xv);
    for (int k = 0; k < n2; ++k) {
      if (k > 0) {
        const float x = xv * rec0[k] * pv - rec1[k] * pv1;
        pv1 = pv;
        pv = x;
      }
      if ((k & (DIF_NW - 1)) != wv) continue;
      const float4* h = reinterpret_cast<const float4*>(Hs + k * n2 * 8);
      float r8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      float pu1 = 0.f, pu = pu0;
      for (int l = 0; l < n2; ++l) {
        if (l > 0) {
          const float x = xu * rec0[l] * pu - rec1[l] * pu1;
          pu1 = pu;
          pu = x;
        }
        const float4 h0 = h[2 * l], h1 = h[2 * l + 1];
        r8[0] += pu * h0.x; r8[1] += pu * h0.y;
        r8[2] += pu * h0.z; r8[3] += pu * h0.w;
        r8[4] += pu * h1.x; r8[5] += pu * h1.y;
        r8[6] += pu * h1.z; r8[7] += pu * h1.w;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) a8[i] += pv * r8[i];
    }
    float4* rp = reinterpret_cast<float4*>(red + (wv * WAVE + lane) * 8);
    rp[0] = {a8[0], a8[1], a8[2], a8[3]};
    rp[1] = {a8[4], a8[5], a8[6], a8[7]};
    __syncthreads();
    if (wv == 0 && live) {
      float4 s0 = rp[0], s1 = rp[1];
#pragma unroll
      for (int x = 1; x < DIF_NW; ++x) {
        const float4 y0 = rp[x * WAVE * 2], y1 = rp[x * WAVE * 2 + 1];
        s0.x += y0.x; s0.y += y0.y; s0.z += y0.z; s0.w += y0.w;
        s1.x += y1.x; s1.y += y1.y; s1.z += y1.z; s1.w += y1.w;
      }
      const double G = phase_term(ur, vr, w[r], ll, mm, nn1);
      float sp, cp;
      sincos_reduced(G * freq, &sp, &cp);
      const double smf = G * fdelta2;
      const float sme = fabs(smf) > 1e-12 ? (float)fabs(sin(smf) / smf) : 1.f;
      const cf ph = {cp * sme, sp * sme};
      const cf o0 = cmul({s0.x, s0.y}, ph), o1 = cmul({s0.z, s0.w}, ph);
      const cf o2 = cmul({s1.x, s1.y}, ph), o3 = cmul({s1.z, s1.w}, ph);
      float4* o = reinterpret_cast<float4*>(out + r * 4);
      o[0] = {o0.x, o0.y, o1.x, o1.y};
      o[1] = {o2.x, o2.y, o3.x, o3.y};
    }
    __syncthreads();
  }
}

extern "C" __global__ void __launch_bounds__(DIF_TB)
k_diffuse_station(DiffuseArgs a) {
  diffuse_station_body(a.Z, a.C, a.T1, a.T2, a.A, a.B, a.Gz, a.Gc);
}

extern "C" __global__ void __launch_bounds__(DIF_TB)
k_diffuse_pair(DiffuseArgs a, float2* out) {
  diffuse_pair_body(a.u, a.v, a.w, a.pairs, a.A, a.B, a.T, a.Nbase, a.Gz,
                    a.Gc, a.g2, a.ll, a.mm, a.nn1, a.freq, a.fdelta2, out);
}
