// Joint cross-cluster normal equations for gfx950 (MI355X): H = J^T W J,
// g = J^T W r and the weighted cost over the FULL parameter vector, what
// reference.joint_jtj_jtr assembles with 5 M^2 index_add_ passes and two
// dense complex accumulators, in two launches and with no intermediate of
// the size of H.
//
// For one station pair b = (p, q) and one timeslot t, with c_i =
// chunk_tab[ci, t], C_i = sqrt(w) cohs[ci, r], row r = t*Nbase + b:
//   G1_i = C_i J[c_i, q]^H,  K_i = J[c_i, p] C_i,
//   res  = sqrt(w) x[r] - sum_i J[c_i, p] G1_i
// (the row weight enters once, as sqrt(w) on x and C: every product below
// is then the unweighted formula). Stack z = [vec G1_0 .. vec G1_{M-1};
// vec K_0 .. vec K_{M-1}] in C^{8M}. Everything the pair adds to H is an
// entry of the Gram matrix S = sum_t z z^H or a trace over one index of it:
//   (p,ci)x(p,cj)  Epp[j,j'] = conj(sum_k G1_i[j,k] conj(G1_j[j',k]))
//   (q,ci)x(q,cj)  Eqq[j,j'] = conj(sum_i conj(K_i[i,j]) K_j[i,j'])
//   (p,ci)x(q,cj)  Cx[(i,j),(k,b)] = conj(G1_i[j,k]) K_j[i,b]
// realified as reference.joint_jtj_jtr's docstring says, and
//   g(c_i, p) += vecR(res G1_i^H),  g(c_i, q) += vecR(res^H K_i).
//
// MFMA or VALU. At M = 10, T = 60 the stacked real form [Re z; Im z] is a
// 160 x 160 x 60 SYRK per pair: 100 tiles of mfma_f32_16x16x4_f32, 15 k
// steps each, 1500 MFMAs of 32 cycles = 48 k SIMD cycles (26 k with the
// lower triangle and the K x G1 quadrant skipped, 55 tiles). Of each 4x4
// complex block of S the closed forms read 8 (Epp: k = k'), 8 (Eqq) and 16
// (Cx) entries, and Epp and Eqq only for ci <= cj: 8 + 8 + 2*16 cmul per
// unordered cluster pair, 2310 cmul per row at M = 10 against 6400 in the
// full Gram. At 4 VALU instructions per cmul and 4 cycles per wave
// instruction that is 60 * 2310 * 4 / 64 * 4 = 35 k SIMD cycles per pair.
// fp32 MFMA and unpacked fp32 FMA both peak at 256 flop/cycle/CU on this
// chip, so the matrix pipe buys nothing for the 2.8 x extra products, and
// it would need z split into real and imaginary planes in LDS plus an
// epilogue that picks the traces back out of the tiles. The closed-form
// VALU route is taken; z still goes through LDS once per timeslot and is
// read from there by every product (broadcast reads: the lanes of a wave
// share t and mostly ci).
//
// k_joint_gram   one workgroup of 128 threads per station pair; a flagged
//                pair (negative entry) leaves at once and looks up nothing.
//                The host cuts the timeslots into pieces: the finest
//                segments over which every cluster's chunk id is constant,
//                cut again at JOINT_JTJ_TT timeslots. The workgroup walks
//                the pieces in order. Per piece: (1) J[c_i, p] and
//                J[c_i, q] of the M chunks in play go to LDS; (2) threads
//                (t, ci) form G1 and K and store z[t][ci][8] to LDS;
//                (3) threads t form res (LDS) and the piece's cost, summed
//                by wave 0's shuffle tree into its own cell of PC
//                [Nbase, E]; (4) threads take work items, each 8 cmul per
//                timeslot with 4 or 8 complex accumulators in registers:
//                  (ci, cj, i)   row i of Cx, all ci, cj      2 M^2 items
//                  (ci<=cj, side) Epp or Eqq                  M (M+1) items
//                  (ci, side)    the gradient of (c_i, p|q)   2 M items
//                331 items at M = 10. A Cx item stores its 4 x 8 reals
//                and their transpose straight into H: block (c_i,p) x
//                (c_j,q) belongs to this pair alone. E and g items store
//                to the pair's own slot of PE [Nbase, D, 2, 4] and PG
//                [Nbase, G, 2, 4], D the distinct (c_i, c_j), ci <= cj,
//                G the chunks in play. The first piece that lands on a
//                destination stores, later ones (hybrid chunks, or a
//                segment longer than the time tile) read, add and store:
//                the same thread each time, in piece order, so the sum has
//                one fixed order and nothing needs clearing.
// k_joint_cost   steps (1)-(3) alone, for the LM trial cost; takes no H.
// k_joint_reduce one wave per (station s, slot): the (pair, side) entries
//                of s (hip_host._lbfgs_stations, sorted by pair) are dealt
//                to the 64 lanes in a fixed order and summed by a butterfly
//                that leaves the same bits in every lane; lane (row, col)
//                stores its element of the realified 8 x 8 block (c_i,s) x
//                (c_j,s) and, off the diagonal, of the transposed block, so
//                H == H^T holds bit for bit (a diagonal block is made
//                Hermitian first: Im E_jj = 0, E_10 = conj E_01). g slots
//                the same way, 8 lanes store. The last blocks sum PC in
//                double per cost bin (one bin, or one per block of the
//                blocked layout).
//
// Layouts. Dense: H [P, P], P = 8 Mt N, row of (chunk c, station s) at
// (c N + s) 8. Blocked: H [Kb, Pb, Pb], Pb = 8 M N; cpos[c] = (block,
// position in block) places chunk c, ld = P or Pb. H and g arrive zeroed;
// the kernels write every structurally non-zero entry.
//
// Partials at 64 stations, 10 clusters, 2016 pairs: one chunk per cluster
// D = 55, G = 10: PE 7.1 MB, PG 1.3 MB; 16 chunks per cluster D = 880,
// G = 160: PE 113.5 MB, PG 20.6 MB, against H of 1.7 GB. LDS: z is
// 32 * M * 64 B, 20 KB at M = 10, which bounds M at 30 under 64 KB.
//
// No float atomics: two evaluations agree bit for bit, as jtj.hip's header
// argues for the LM accept/reject chain.
#include "common.h"

#define JJ_TB JOINT_JTJ_TB
#define JJ_TT JOINT_JTJ_TT
static_assert(JJ_TT <= WAVE, "the piece cost is summed inside wave 0");
// compiled without packed fp32 arithmetic, like lbfgs_mf.hip
#define JJ_KERNEL \
  extern "C" __global__ void __attribute__((target("no-packed-fp32-ops")))

__device__ __forceinline__ void jj_load4(const cf* __restrict__ a, size_t row,
                                         cf* m) {
  const float4* v = reinterpret_cast<const float4*>(a + row * 4);
  const float4 lo = v[0], hi = v[1];
  m[0] = {lo.x, lo.y}; m[1] = {lo.z, lo.w};
  m[2] = {hi.x, hi.y}; m[3] = {hi.z, hi.w};
}

__device__ __forceinline__ void jj_store4(cf* __restrict__ a, size_t row,
                                          const cf* m) {
  float4* v = reinterpret_cast<float4*>(a + row * 4);
  v[0] = make_float4(m[0].x, m[0].y, m[1].x, m[1].y);
  v[1] = make_float4(m[2].x, m[2].y, m[3].x, m[3].y);
}

// store, or add to what an earlier piece of this pair left there
__device__ __forceinline__ void jj_commit4(cf* __restrict__ a, size_t row,
                                           cf* m, bool first) {
  if (!first) {
    cf old[4];
    jj_load4(a, row, old);
#pragma unroll
    for (int i = 0; i < 4; ++i) m[i] = cadd(m[i], old[i]);
  }
  jj_store4(a, row, m);
}

__device__ __forceinline__ float4 jj_add(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// the same bits in every lane: a + b and b + a round alike
__device__ __forceinline__ float jj_wave_all(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE);
  return x;
}

__device__ __forceinline__ double jj_wave_all(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE);
  return x;
}

// index of (a, b), a <= b, in the row-major upper triangle of M x M
__device__ __forceinline__ int jj_tri(int a, int b, int M) {
  return a * M - a * (a - 1) / 2 + (b - a);
}

__device__ __forceinline__ void joint_gram_body(
    const cf* __restrict__ x, const cf* __restrict__ cohs,
    const cf* __restrict__ J, const float* __restrict__ wts,
    const int* __restrict__ pairs, const int* __restrict__ chunk_tab,
    const int* __restrict__ pieces, const int* __restrict__ etab,
    const int* __restrict__ gtab, const int* __restrict__ cpos, int M, int T,
    int Nbase, int N, int E, int D, int G, long long ld, const bool cost_only,
    float* __restrict__ H, cf* __restrict__ PE, cf* __restrict__ PG,
    float* __restrict__ PC) {
  extern __shared__ float4 jj_lds[];
  cf* Z = reinterpret_cast<cf*>(jj_lds);      // [TT][M][8]: G1 then K
  cf* Rr = Z + (size_t)JJ_TT * M * 8;         // [TT][4]: res
  cf* JJ = Rr + JJ_TT * 4;                    // [2][M][4]: J[c_i,p], J[c_i,q]
  const int b = blockIdx.x;
  const int p = pairs[2 * b], q = pairs[2 * b + 1];
  if (p < 0 || q < 0) return;                 // flagged: nothing reads its slots
  const int tid = threadIdx.x;
  const size_t R = (size_t)T * Nbase;
  const int ntri = M * (M + 1) / 2;
  const int nX = 2 * M * M, nE = 2 * ntri;
  const int nitems = cost_only ? 0 : nX + nE + 2 * M;
  for (int e = 0; e < E; ++e) {
    const int t0 = pieces[2 * e], nt = pieces[2 * e + 1] - t0;
    if (tid < 2 * M) {
      const int side = tid / M, ci = tid - side * M;
      const int c = chunk_tab[(size_t)ci * T + t0];
      jj_load4(J, (size_t)c * N + (side ? q : p), JJ + tid * 4);
    }
    __syncthreads();
    for (int it = tid; it < nt * M; it += JJ_TB) {
      const int tl = it / M, ci = it - tl * M;
      const size_t r = (size_t)(t0 + tl) * Nbase + b;
      cf C[4], G1[4], K[4];
      jj_load4(cohs, (size_t)ci * R + r, C);
      if (wts != nullptr) {
        const float sw = sqrtf(wts[r]);
#pragma unroll
        for (int i = 0; i < 4; ++i) C[i] = cscale(C[i], sw);
      }
      m2mulh(C, JJ + (M + ci) * 4, G1);       // G1 = C J_q^H
      m2mul(JJ + ci * 4, C, K);               // K  = J_p C
      jj_store4(Z, (size_t)it * 2, G1);
      jj_store4(Z, (size_t)it * 2 + 1, K);
    }
    __syncthreads();
    if (tid < WAVE) {                         // wave 0, whole
      float e2 = 0.f;
      if (tid < nt) {
        const size_t r = (size_t)(t0 + tid) * Nbase + b;
        cf res[4];
        jj_load4(x, r, res);
        if (wts != nullptr) {
          const float sw = sqrtf(wts[r]);
#pragma unroll
          for (int i = 0; i < 4; ++i) res[i] = cscale(res[i], sw);
        }
        for (int ci = 0; ci < M; ++ci) {
          cf V[4];
          m2mul(JJ + ci * 4, Z + ((size_t)tid * M + ci) * 8, V);
#pragma unroll
          for (int i = 0; i < 4; ++i) res[i] = csub(res[i], V[i]);
        }
        jj_store4(Rr, tid, res);
        e2 = cabs2(res[0]) + cabs2(res[1]) + cabs2(res[2]) + cabs2(res[3]);
      }
      e2 = jj_wave_all(e2);
      if (tid == 0) PC[(size_t)b * E + e] = e2;
    }
    __syncthreads();
    for (int id = tid; id < nitems; id += JJ_TB) {
      if (id < nX) {
        // row i of Cx(ci, cj): acc[(2j+k)*2 + b] = sum K_j[i,b] conj G1_i[j,k]
        const int ci = id / (2 * M), rem = id - ci * 2 * M;
        const int cj = rem >> 1, i = rem & 1;
        cf acc[8] = {};
        for (int tl = 0; tl < nt; ++tl) {
          const cf* g1 = Z + ((size_t)tl * M + ci) * 8;
          const cf* k = Z + ((size_t)tl * M + cj) * 8 + 4 + 2 * i;
#pragma unroll
          for (int jk = 0; jk < 4; ++jk) {
            acc[2 * jk] = cadd(acc[2 * jk], cmulc(k[0], g1[jk]));
            acc[2 * jk + 1] = cadd(acc[2 * jk + 1], cmulc(k[1], g1[jk]));
          }
        }
        const int c1 = chunk_tab[(size_t)ci * T + t0];
        const int c2 = chunk_tab[(size_t)cj * T + t0];
        const bool first =
            etab[(size_t)e * ntri + (ci <= cj ? jj_tri(ci, cj, M)
                                              : jj_tri(cj, ci, M))] & 1;
        float* Hb = H + (size_t)cpos[2 * c1] * ld * ld;
        const size_t row0 = ((size_t)cpos[2 * c1 + 1] * N + p) * 8 + 4 * i;
        const size_t col0 = ((size_t)cpos[2 * c2 + 1] * N + q) * 8;
        // rows (j, re|im) of the anti-linear 2x2s [[cr, ci], [ci, -cr]]
        float4 v[4][2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            const cf a0 = acc[(2 * j + k) * 2], a1 = acc[(2 * j + k) * 2 + 1];
            v[2 * j][k] = make_float4(a0.x, a0.y, a1.x, a1.y);
            v[2 * j + 1][k] = make_float4(a0.y, -a0.x, a1.y, -a1.x);
          }
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          float4* dst = reinterpret_cast<float4*>(Hb + (row0 + r4) * ld + col0);
          if (!first) {
            v[r4][0] = jj_add(v[r4][0], dst[0]);
            v[r4][1] = jj_add(v[r4][1], dst[1]);
          }
          dst[0] = v[r4][0];
          dst[1] = v[r4][1];
        }
        // the transposed block (c_j,q) x (c_i,p): the summed values again
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          float* tp = Hb + (col0 + 4 * k) * ld + row0;
          *reinterpret_cast<float4*>(tp) =
              make_float4(v[0][k].x, v[1][k].x, v[2][k].x, v[3][k].x);
          *reinterpret_cast<float4*>(tp + ld) =
              make_float4(v[0][k].y, v[1][k].y, v[2][k].y, v[3][k].y);
          *reinterpret_cast<float4*>(tp + 2 * ld) =
              make_float4(v[0][k].z, v[1][k].z, v[2][k].z, v[3][k].z);
          *reinterpret_cast<float4*>(tp + 3 * ld) =
              make_float4(v[0][k].w, v[1][k].w, v[2][k].w, v[3][k].w);
        }
      } else if (id < nX + nE) {
        const int side = (id - nX) & 1;
        int tri = (id - nX) >> 1, ci = 0;
        while (tri >= M - ci) { tri -= M - ci; ++ci; }
        const int cj = ci + tri;
        cf acc[4] = {};
        if (side == 0) {                      // A[j][j'] = G1_i G1_j^H
          for (int tl = 0; tl < nt; ++tl) {
            cf t4[4];
            m2mulh(Z + ((size_t)tl * M + ci) * 8,
                   Z + ((size_t)tl * M + cj) * 8, t4);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = cadd(acc[i], t4[i]);
          }
        } else {                              // A[j][j'] = K_i^H K_j
          for (int tl = 0; tl < nt; ++tl) {
            cf t4[4];
            m2hmul(Z + ((size_t)tl * M + ci) * 8 + 4,
                   Z + ((size_t)tl * M + cj) * 8 + 4, t4);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = cadd(acc[i], t4[i]);
          }
        }
        // Epp = conj(G1_i G1_j^H); Eqq = conj(K_i^H K_j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = conjf2(acc[i]);
        const int sl = etab[(size_t)e * ntri + jj_tri(ci, cj, M)];
        jj_commit4(PE, ((size_t)b * D + (sl >> 1)) * 2 + side, acc, sl & 1);
      } else {
        const int side = (id - nX - nE) & 1, ci = (id - nX - nE) >> 1;
        cf acc[4] = {};
        if (side == 0) {                      // res G1^H
          for (int tl = 0; tl < nt; ++tl) {
            cf t4[4];
            m2mulh(Rr + tl * 4, Z + ((size_t)tl * M + ci) * 8, t4);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = cadd(acc[i], t4[i]);
          }
        } else {                              // res^H K
          for (int tl = 0; tl < nt; ++tl) {
            cf t4[4];
            m2hmul(Rr + tl * 4, Z + ((size_t)tl * M + ci) * 8 + 4, t4);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = cadd(acc[i], t4[i]);
          }
        }
        const int gs = gtab[(size_t)e * M + ci];
        jj_commit4(PG, ((size_t)b * G + (gs >> 1)) * 2 + side, acc, gs & 1);
      }
    }
    __syncthreads();                          // Z, Rr, JJ are rewritten next
  }
}

JJ_KERNEL __launch_bounds__(JJ_TB)
k_joint_gram(JointJtjArgs a, float* H, float2* PE, float2* PG, float* PC) {
  joint_gram_body(a.x, a.cohs, a.J, a.wts, a.pairs, a.chunk_tab, a.pieces,
                  a.etab, a.gtab, a.cpos, a.M, a.T, a.Nbase, a.N, a.E, a.D,
                  a.G, a.ld, false, H, PE, PG, PC);
}

JJ_KERNEL __launch_bounds__(JJ_TB)
k_joint_cost(JointJtjArgs a, float* PC) {
  joint_gram_body(a.x, a.cohs, a.J, a.wts, a.pairs, a.chunk_tab, a.pieces,
                  nullptr, nullptr, nullptr, a.M, a.T, a.Nbase, a.N, a.E, 0, 0,
                  0, true, nullptr, nullptr, nullptr, PC);
}

// bin k of the cost: the pieces with cbin == k over the unflagged pairs
__device__ __forceinline__ void joint_cost_bin(
    const float* __restrict__ PC, const int* __restrict__ cbin,
    const int* __restrict__ pairs, int E, int Nbase, int k,
    float* __restrict__ cost) {
  const int lane = threadIdx.x;
  double s = 0.0;
  const long long items = (long long)E * Nbase;
  for (long long i = lane; i < items; i += WAVE) {
    const int e = (int)(i / Nbase), b = (int)(i - (long long)e * Nbase);
    if (cbin[e] == k && pairs[2 * b] >= 0 && pairs[2 * b + 1] >= 0)
      s += (double)PC[(size_t)b * E + e];
  }
  s = jj_wave_all(s);
  if (lane == 0) cost[k] = (float)s;
}

__device__ __forceinline__ void joint_reduce_body(
    const cf* __restrict__ PE, const cf* __restrict__ PG,
    const float* __restrict__ PC, const int* __restrict__ pairs,
    const int* __restrict__ cbin, const int* __restrict__ sdst,
    const int* __restrict__ gdst, const int* __restrict__ cpos,
    const int* __restrict__ sta_off, const int* __restrict__ sta_ent,
    int Nbase, int N, int E, int D, int G, long long ld,
    float* __restrict__ H, float* __restrict__ g, float* __restrict__ cost) {
  const int lane = threadIdx.x;
  const long long nslot = (long long)N * (D + G);
  if ((long long)blockIdx.x >= nslot) {
    joint_cost_bin(PC, cbin, pairs, E, Nbase, (int)(blockIdx.x - nslot), cost);
    return;
  }
  const int s = blockIdx.x / (D + G), sl = blockIdx.x - s * (D + G);
  const int k0 = sta_off[s], nk = sta_off[s + 1] - k0;
  const bool is_g = sl >= D;
  const cf* P = is_g ? PG : PE;
  const int nsl = is_g ? G : D, slot = is_g ? sl - D : sl;
  cf a[4] = {};
  for (int k = lane; k < nk; k += WAVE) {
    const int ent = sta_ent[k0 + k];          // 2*b + side
    cf t4[4];
    jj_load4(P, ((size_t)(ent >> 1) * nsl + slot) * 2 + (ent & 1), t4);
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = cadd(a[i], t4[i]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a[i].x = jj_wave_all(a[i].x);
    a[i].y = jj_wave_all(a[i].y);
  }
  if (is_g) {
    const int c = gdst[slot];
    if (lane < 8) {
      const cf v = a[lane >> 1];
      g[(size_t)cpos[2 * c] * ld + ((size_t)cpos[2 * c + 1] * N + s) * 8 +
        lane] = (lane & 1) ? v.y : v.x;
    }
    return;
  }
  const int c1 = sdst[2 * slot], c2 = sdst[2 * slot + 1];
  if (c1 == c2) {                             // Hermitian, to the last bit
    a[0].y = 0.f;
    a[3].y = 0.f;
    a[2] = conjf2(a[1]);
  }
  // element (r8, c8) of I2 (x) realify(E): r8 = 4i + 2j + re|im
  const int r8 = lane >> 3, c8 = lane & 7;
  const cf el = a[((r8 >> 1) & 1) * 2 + ((c8 >> 1) & 1)];
  float val = 0.f;
  if ((r8 >> 2) == (c8 >> 2))
    val = (r8 & 1) == (c8 & 1) ? el.x : ((r8 & 1) ? el.y : -el.y);
  float* Hb = H + (size_t)cpos[2 * c1] * ld * ld;
  const size_t row = ((size_t)cpos[2 * c1 + 1] * N + s) * 8 + r8;
  const size_t col = ((size_t)cpos[2 * c2 + 1] * N + s) * 8 + c8;
  Hb[row * ld + col] = val;
  if (c1 != c2) Hb[col * ld + row] = val;
}

JJ_KERNEL __launch_bounds__(WAVE)
k_joint_reduce(JointJtjArgs a, const float2* PE, const float2* PG,
               const float* PC, float* H, float* g, float* cost) {
  joint_reduce_body(PE, PG, PC, a.pairs, a.cbin, a.sdst, a.gdst, a.cpos,
                    a.sta_off, a.sta_ent, a.Nbase, a.N, a.E, a.D, a.G, a.ld,
                    H, g, cost);
}

// the cost bins alone, after k_joint_cost
JJ_KERNEL __launch_bounds__(WAVE)
k_joint_cost_reduce(JointJtjArgs a, const float* PC, float* cost) {
  joint_cost_bin(PC, a.cbin, a.pairs, a.E, a.Nbase, blockIdx.x, cost);
}
