// Multi-channel LBFGS cost and gradient for gfx950 (MI355X): the role of
// the reference's fused multi-frequency gradient (lbfgs_multifreq.cu
// kernel_deriv_r_robust), in three launches whatever the number of channels
// F and clusters M, with no per-cluster intermediate.
//
// With (p, q) = pairs[b], c = chunk_tab[ci, t], J1 = J[c, p], J2 = J[c, q],
// C = cohs[f, ci, r] and rows r = t*Nbase + b:
//   res = xs[f, r] - sum_ci J1 C J2^H,  e2 = |res|_F^2
//   Gaussian: cost = sum e2, s = 1; robust: cost = sum log1p(e2 / nu),
//   s = 1 / (nu + e2)
//   grad(c, p) = -2 vecR(sum s res G1^H), G1 = C J2^H
//   grad(c, q) = -2 vecR(sum s res^H K),  K  = J1 C
//
// k_lbfgs_mf_res     one thread per (f, row), 256 per workgroup, channels
//                    along blockIdx.y. Loops over the clusters (k_apply_
//                    jones's order: C J2^H, then J1 times it), forms res,
//                    e2, the cost term and s, and stores s*res [F, R, 4],
//                    zeros on a row whose pair has a negative entry. The
//                    workgroup's cost terms are summed in a fixed order
//                    (shuffle tree, then the four waves in turn) into its
//                    own cell of cpart [F, blocks]. J is gathered from
//                    global memory here: a workgroup's 256 rows may lie in
//                    several timeslots and so in several chunks.
// k_lbfgs_mf_grad    lanes run along the baseline axis: thread <-> pair
//                    b = blockIdx.y*256 + tid, so a wave reads 64
//                    consecutive rows of one (f, ci, t), 2 KB contiguous of
//                    s*res and of cohs. A workgroup owns that tile of 256
//                    consecutive pairs and one extent (ci, c, t0, t1): a run
//                    of timeslots of cluster ci that all lie in chunk c.
//                    It walks (t, f) over the extent with gp[4], gq[4] of
//                    its pair in registers and commits them with plain
//                    stores to the pair's own slot [extent, pair, 8].
//                    LDS holds J[c, :, :] of the extent's chunk, N*32 bytes
//                    (2 KB at 64 stations, 16 KB at 512), staged once per
//                    workgroup; each thread takes its J1 and J2 from there,
//                    indexed by p and q. A chunk never changes inside a
//                    workgroup's walk: the host cuts every cluster's row of
//                    chunk_tab into runs of one chunk id, and runs longer
//                    than the time split into pieces, each an extent with a
//                    slot row of its own (hip_host._lbfgs_tables, once per
//                    table). A chunk id that comes back later in time is
//                    simply another extent of that chunk.
// k_lbfgs_mf_reduce  block (c, s): the extents of chunk c (ext_off, the
//                    extent list is sorted by chunk) times the (pair, side)
//                    entries of station s (sta_off / sta_ent, sorted by
//                    pair) are dealt to the 64 lanes in a fixed order and
//                    summed by the fixed shuffle tree; lane 0 stores
//                    -2 * the sum as the 8 floats of grad[c, s]. Every
//                    (c, s) is written, zeros for a station without
//                    baselines or a chunk without extents, so grad needs no
//                    clearing. The last block sums cpart in double, in a
//                    fixed order, into the scalar cost.
//
// No float atomics anywhere, cost included: the result repeats bit for bit,
// which jtj.hip's header argues for the LM accept/reject chain and which
// holds for an LBFGS line search alike.
//
// No matrix instructions: the arithmetic is five 2x2 complex products per
// row and cluster against 64 bytes read, about 1.7 flop per byte; the
// kernels are bandwidth-bound and MFMA has nothing to feed on.
//
// hipcc -O3 for gfx950, -Rpass-analysis=kernel-resource-usage:
//                      VGPRs  SGPRs  LDS            waves per SIMD
//   k_lbfgs_mf_res       55     49   16 B (static)        8
//   k_lbfgs_mf_grad     122     45   N*32 B (dynamic)     4
//   k_lbfgs_mf_reduce    26     43   0                    8
// no scratch in any of them. The gradient kernel's registers are the two
// channels of its unrolled inner loop in flight, 64 bytes of loads per lane
// each.
#include "common.h"

#define LMF_TB LBFGS_MF_TB
// The three kernels are compiled without packed fp32 arithmetic: left to
// itself the compiler pairs the complex products into two-lane packed
// multiplies and adds, forms this code does not rely on for gfx950.
#define LMF_KERNEL \
  extern "C" __global__ void __attribute__((target("no-packed-fp32-ops")))

// one 2x2 complex matrix, two 16-byte loads
__device__ __forceinline__ void lmf_load4(const float2* __restrict__ a,
                                          size_t row, cf* m) {
  const float4* v = reinterpret_cast<const float4*>(a + row * 4);
  const float4 lo = v[0], hi = v[1];
  m[0] = {lo.x, lo.y}; m[1] = {lo.z, lo.w};
  m[2] = {hi.x, hi.y}; m[3] = {hi.z, hi.w};
}

__device__ __forceinline__ void lmf_store4(float2* __restrict__ a, size_t row,
                                           const cf* m) {
  float4* v = reinterpret_cast<float4*>(a + row * 4);
  v[0] = make_float4(m[0].x, m[0].y, m[1].x, m[1].y);
  v[1] = make_float4(m[2].x, m[2].y, m[3].x, m[3].y);
}

__device__ __forceinline__ float lmf_wave_sum(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, WAVE);
  return x;
}

__device__ __forceinline__ double lmf_wave_sum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, WAVE);
  return x;
}

__device__ __forceinline__ void lbfgs_mf_res_body(
    const float2* __restrict__ xs, const float2* __restrict__ cohs,
    const float2* __restrict__ J, const int* __restrict__ pairs,
    const int* __restrict__ chunk_tab, int M, int T, int Nbase, int N,
    float nu, float2* __restrict__ sres, float* __restrict__ cpart) {
  __shared__ float ws[LMF_TB / WAVE];
  const size_t R = (size_t)T * Nbase;
  const size_t r = (size_t)blockIdx.x * LMF_TB + threadIdx.x;
  const int f = blockIdx.y;
  float term = 0.f;
  if (r < R) {
    const int t = (int)(r / Nbase);
    const int b = (int)(r - (size_t)t * Nbase);
    const int p = pairs[2 * b], q = pairs[2 * b + 1];
    cf res[4] = {};
    if (p >= 0 && q >= 0) {
      lmf_load4(xs, (size_t)f * R + r, res);
      for (int ci = 0; ci < M; ++ci) {
        const int c = chunk_tab[(size_t)ci * T + t];
        cf J1[4], J2[4], C[4], G1[4], V[4];
        lmf_load4(J, (size_t)c * N + p, J1);
        lmf_load4(J, (size_t)c * N + q, J2);
        lmf_load4(cohs, ((size_t)f * M + ci) * R + r, C);
        m2mulh(C, J2, G1);
        m2mul(J1, G1, V);
#pragma unroll
        for (int i = 0; i < 4; ++i) res[i] = csub(res[i], V[i]);
      }
      const float e2 = cabs2(res[0]) + cabs2(res[1]) + cabs2(res[2]) +
                       cabs2(res[3]);
      float s = 1.f;
      term = e2;
      if (nu > 0.f) {
        term = log1pf(e2 / nu);
        s = 1.f / (nu + e2);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) res[i] = cscale(res[i], s);
    }
    lmf_store4(sres, (size_t)f * R + r, res);
  }
  term = lmf_wave_sum(term);
  if ((threadIdx.x & (WAVE - 1)) == 0) ws[threadIdx.x / WAVE] = term;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < LMF_TB / WAVE; ++i) tot += ws[i];
    cpart[(size_t)f * gridDim.x + blockIdx.x] = tot;
  }
}

LMF_KERNEL __launch_bounds__(LMF_TB)
k_lbfgs_mf_res(LbfgsMfArgs a, float2* sres, float* cpart) {
  lbfgs_mf_res_body(a.xs, a.cohs, a.J, a.pairs, a.chunk_tab, a.M, a.T,
                    a.Nbase, a.N, a.nu, sres, cpart);
}

__device__ __forceinline__ void lbfgs_mf_grad_body(
    const float2* __restrict__ sres, const float2* __restrict__ cohs,
    const float2* __restrict__ J, const int* __restrict__ pairs,
    const int4* __restrict__ ext, int F, int M, int T, int Nbase, int N,
    float2* __restrict__ slots) {
  extern __shared__ float4 lmf_J[];     // [N][2]: J[c, :, :]
  const int e = blockIdx.x;
  const int4 x = ext[e];                // ci, c, t0, t1
  const float4* Jc = reinterpret_cast<const float4*>(J) + (size_t)x.y * N * 2;
  for (int i = threadIdx.x; i < 2 * N; i += LMF_TB) lmf_J[i] = Jc[i];
  __syncthreads();
  const int b = blockIdx.y * LMF_TB + threadIdx.x;
  if (b >= Nbase) return;
  const int p = pairs[2 * b], q = pairs[2 * b + 1];
  if (p < 0 || q < 0) return;           // flagged: no entry reads this slot
  cf J1[4], J2[4];
  lmf_load4(reinterpret_cast<const float2*>(lmf_J), p, J1);
  lmf_load4(reinterpret_cast<const float2*>(lmf_J), q, J2);
  const size_t R = (size_t)T * Nbase;
  cf gp[4] = {}, gq[4] = {};
  for (int t = x.z; t < x.w; ++t) {
    const size_t r = (size_t)t * Nbase + b;
#pragma unroll 2
    for (int f = 0; f < F; ++f) {
      cf S[4], C[4], G1[4], K[4], t4[4];
      lmf_load4(sres, (size_t)f * R + r, S);
      lmf_load4(cohs, ((size_t)f * M + x.x) * R + r, C);
      m2mulh(C, J2, G1);                // G1 = C J2^H
      m2mul(J1, C, K);                  // K  = J1 C
      m2mulh(S, G1, t4);                // gp += s res G1^H
#pragma unroll
      for (int i = 0; i < 4; ++i) gp[i] = cadd(gp[i], t4[i]);
      m2hmul(S, K, t4);                 // gq += s res^H K
#pragma unroll
      for (int i = 0; i < 4; ++i) gq[i] = cadd(gq[i], t4[i]);
    }
  }
  const size_t slot = ((size_t)e * Nbase + b) * 2;   // unique writer
  lmf_store4(slots, slot, gp);
  lmf_store4(slots, slot + 1, gq);
}

LMF_KERNEL __launch_bounds__(LMF_TB)
k_lbfgs_mf_grad(LbfgsMfArgs a, const float2* sres, float2* slots) {
  lbfgs_mf_grad_body(sres, a.cohs, a.J, a.pairs,
                     reinterpret_cast<const int4*>(a.ext), a.F, a.M, a.T,
                     a.Nbase, a.N, slots);
}

__device__ __forceinline__ void lbfgs_mf_reduce_body(
    const float2* __restrict__ slots, const float* __restrict__ cpart,
    const int* __restrict__ ext_off, const int* __restrict__ sta_off,
    const int* __restrict__ sta_ent, int Nbase, int N, int Mt,
    long long ncpart, float* __restrict__ grad, float* __restrict__ cost) {
  const int lane = threadIdx.x;
  if (blockIdx.x == (unsigned)Mt * N) {
    double s = 0.0;
    for (long long i = lane; i < ncpart; i += WAVE) s += (double)cpart[i];
    s = lmf_wave_sum(s);
    if (lane == 0) *cost = (float)s;
    return;
  }
  const int c = blockIdx.x / N, s = blockIdx.x - c * N;
  const int e0 = ext_off[c], ne = ext_off[c + 1] - e0;
  const int k0 = sta_off[s], nk = sta_off[s + 1] - k0;
  cf g[4] = {};
  if (nk > 0) {
    const long long items = (long long)ne * nk;
    for (long long it = lane; it < items; it += WAVE) {
      const int e = e0 + (int)(it / nk);
      const int ent = sta_ent[k0 + (int)(it % nk)];   // 2*b + side
      cf a[4];
      lmf_load4(slots, ((size_t)e * Nbase + (ent >> 1)) * 2 + (ent & 1), a);
#pragma unroll
      for (int i = 0; i < 4; ++i) g[i] = cadd(g[i], a[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    g[i].x = lmf_wave_sum(g[i].x);
    g[i].y = lmf_wave_sum(g[i].y);
  }
  if (lane == 0) {
    float* o = grad + (size_t)blockIdx.x * 8;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      o[2 * i] = -2.f * g[i].x;
      o[2 * i + 1] = -2.f * g[i].y;
    }
  }
}

LMF_KERNEL __launch_bounds__(WAVE)
k_lbfgs_mf_reduce(LbfgsMfArgs a, const float2* slots, const float* cpart,
                  long long ncpart, float* grad, float* cost) {
  lbfgs_mf_reduce_body(slots, cpart, a.ext_off, a.sta_off, a.sta_ent, a.Nbase,
                       a.N, a.Mt, ncpart, grad, cost);
}
