// The RTR truncated-CG inner solve for gfx950 (MI355X): per chunk, what
// rtr._Objective.grad, rtr._tcg_fixed and the hess_vec(J, eta) after it
// compute with about 40 torch launches per CG iteration, in ONE launch.
//
// One workgroup of RTR_TCG_TB = 1024 threads (16 waves) owns one chunk for
// the whole solve; grid = nchunk. Nothing crosses workgroups: no cooperative
// launch, no flags, no atomics.
//
// With P = 8 N real parameters in reference.vecR order (station, row-major
// 2x2, re/im), the stacked X of rtr._to_X is [2N, 2] complex, and one of its
// rows is one float4 "quad" q = 2 s + i of the parameter vector.
//
// Matvec (the only global reads inside the loop). Wave w takes the row
// groups w, w + 16, ... of 4 consecutive rows of JtJ. Its lanes run along
// the rows with float4 loads, lane l at columns 4 l + 256 k, so consecutive
// lanes read consecutive 16 bytes and the four rows give four independent
// loads per pass. v comes from LDS as one float4 per pass. Each row sum is
// reduced by a 6-step xor butterfly (one fixed order, the same bits in every
// lane); lanes 0..3 scale their row by 2 iw[row / 8] and store Hv to LDS:
// the scalings and the store are the matvec's epilogue. P is a multiple of
// 8, so neither the float4 columns nor the groups of 4 rows have a tail;
// any P = 8 N up to RTR_TCG_MAXP works, multiple of 256 or not.
// JtJ is read in full: reading one triangle would make each lane gather a
// column at stride P floats for the mirrored half, which is not coalesced.
//
// MFMA does not fit: a matrix-vector product does 2 flop per 4-byte element
// of JtJ, 0.5 flop/byte, with no reuse of a loaded element, and an MFMA
// tile earns its rate only by reusing its operands over a second matrix
// dimension that one vector does not have. The kernel is bound by the
// 13 * 4 P^2 bytes per chunk that the 12 + 1 matvecs stream.
//
// Where the vectors live - a change from "all vectors in LDS", for LDS
// space and to make the projection thread-local. Thread q < 2N owns quad q
// of eta, r, d, Hd, g and J in REGISTERS (RTR_TCG_TB >= 2 N at the largest
// P, so one quad per thread is all there is). Only the two vectors that
// change owner pass through LDS: v (quad owner -> every wave) and Hv (row
// owner -> quad owner). That is (2 P + N) floats, 34 KB at P = 4096, where
// six vectors in LDS would need 96 KB; and Z - J Om for quad q needs X row
// q and Om only, so it happens in the owner's registers.
//
// Projection (rtr._proj). X^H X is summed once per launch, J being fixed;
// thread 0 forms its eigendecomposition as rtr._herm2_eig does, same clamps,
// and leaves lam and U in LDS. Per projection the 2x2 complex X^H Z is one
// 8-value workgroup reduction; every thread then forms the same Om from the
// same 8 sums (about 100 flops, cheaper than a broadcast with its barrier).
//
// Reductions: per value a xor butterfly inside each wave, lane 0 to LDS,
// barrier, then every thread adds the 16 wave sums in index order, barrier.
// Every thread holds the same bits, so `done` is uniform over the workgroup
// and leaving the loop early is safe; two launches on the same input agree
// bit for bit.
//
// The loop follows rtr._tcg_fixed statement for statement (metric
// 2 Re tr(a^H b)); a chunk that sets `done` has eta frozen in the torch
// code, so the kernel leaves the loop there. stats = (<g,g>, <g,eta>,
// <eta,Heta>, CG iterations entered).
//
// Compiler report for gfx950 (-Rpass-analysis=kernel-resource-usage),
// k_rtr_tcg: VGPRs 100, AGPRs 0, SGPRs 53, scratch 0 bytes/lane, no spills,
// no dynamic stack, occupancy 4 waves/SIMD (the 16 waves of one workgroup),
// static LDS 560 bytes plus (2 P + N) * 4 dynamic. The sum over the wave
// partials is unrolled by 2 only and the matvec's column loop not at all:
// fully unrolled they spilled 46 VGPRs at the 128 a 1024-thread block gets.
#include "common.h"

#define RT_TB RTR_TCG_TB
#define RT_NW (RT_TB / WAVE)
#define RT_RED 8                    // most values of one reduction
static_assert(RT_TB * 4 >= RTR_TCG_MAXP, "one quad per thread");
// compiled without packed fp32 arithmetic, like joint_jtj.hip
#define RT_KERNEL \
  extern "C" __global__ void __attribute__((target("no-packed-fp32-ops")))

__device__ __forceinline__ float rt_dot(float4 a, float4 b) {
  return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
}

// a + s b
__device__ __forceinline__ float4 rt_axpy(float4 a, float s, float4 b) {
  return make_float4(a.x + s * b.x, a.y + s * b.y, a.z + s * b.z,
                     a.w + s * b.w);
}

// the same bits in every lane: a + b and b + a round alike
__device__ __forceinline__ float rt_wave_all(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE);
  return x;
}

// v[k] summed over the workgroup, left in every thread; whole workgroup
template <int K>
__device__ __forceinline__ void rt_reduce(float (&v)[K], float* red) {
  static_assert(K <= RT_RED, "red holds RT_RED values per wave");
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    v[k] = rt_wave_all(v[k]);
    if (lane == 0) red[wave * RT_RED + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = 0.f;
#pragma unroll 2
  for (int w = 0; w < RT_NW; ++w)
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += red[w * RT_RED + k];
  __syncthreads();                  // red is rewritten by the next call
}

// hb[row] = 2 iw[row / 8] (A vb)[row]; whole workgroup, barriers by caller
__device__ __forceinline__ void rt_matvec(const float* __restrict__ A,
                                          const float* vb, float* hb,
                                          const float* iws, int P) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  for (int gi = wave; gi < P / 4; gi += RT_NW) {
    const float* row = A + (size_t)gi * 4 * P;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 1
    for (int c = lane * 4; c < P; c += WAVE * 4) {
      const float4 v = *reinterpret_cast<const float4*>(vb + c);
      const float4 r0 = *reinterpret_cast<const float4*>(row + c);
      const float4 r1 = *reinterpret_cast<const float4*>(row + P + c);
      const float4 r2 = *reinterpret_cast<const float4*>(row + 2 * P + c);
      const float4 r3 = *reinterpret_cast<const float4*>(row + 3 * P + c);
      a0 += rt_dot(r0, v);
      a1 += rt_dot(r1, v);
      a2 += rt_dot(r2, v);
      a3 += rt_dot(r3, v);
    }
    a0 = rt_wave_all(a0);
    a1 = rt_wave_all(a1);
    a2 = rt_wave_all(a2);
    a3 = rt_wave_all(a3);
    if (lane < 4) {
      const float a = lane == 0 ? a0 : lane == 1 ? a1 : lane == 2 ? a2 : a3;
      const int r = gi * 4 + lane;
      hb[r] = (2.f * a) * iws[r >> 3];
    }
  }
}

// rtr._herm2_eig of S = [[a, b], [conj b, d]]: eig = lam[2], then U[4]
__device__ __forceinline__ void rt_herm2_eig(float a, float d, cf b,
                                             float* eig) {
  const float tr = a + d, hd = (a - d) * 0.5f;
  const float disc = sqrtf(hd * hd + cabs2(b));
  const float l1 = 0.5f * tr + disc, l2 = 0.5f * tr - disc;
  const bool bz = hypotf(b.x, b.y) < 1e-30f;
  cf v1a = bz ? cf{1.f, 0.f} : b;
  cf v1b = bz ? cf{0.f, 0.f} : cf{l1 - a, 0.f};
  const float inv = 1.f / fmaxf(sqrtf(cabs2(v1a) + cabs2(v1b)), 1e-30f);
  v1a = cscale(v1a, inv);
  v1b = cscale(v1b, inv);
  eig[0] = l1; eig[1] = l2;
  cf* U = reinterpret_cast<cf*>(eig + 2);
  U[0] = v1a; U[1] = {-v1b.x, v1b.y};     // [v1a, -conj v1b]
  U[2] = v1b; U[3] = conjf2(v1a);         // [v1b,  conj v1a]
}

// rtr._proj for the quad z of this thread (zero outside the 2N quads), x
// its row of X; whole workgroup
__device__ __forceinline__ float4 rt_proj(float4 z, float4 x, const float* eig,
                                          float* red) {
  const cf x0 = {x.x, x.y}, x1 = {x.z, x.w}, z0 = {z.x, z.y}, z1 = {z.z, z.w};
  // X^H Z, [a][b] = sum conj(X[q, a]) Z[q, b]
  const cf p00 = cmulc(z0, x0), p01 = cmulc(z1, x0);
  const cf p10 = cmulc(z0, x1), p11 = cmulc(z1, x1);
  float s[8] = {p00.x, p00.y, p01.x, p01.y, p10.x, p10.y, p11.x, p11.y};
  rt_reduce(s, red);
  const cf XZ[4] = {{s[0], s[1]}, {s[2], s[3]}, {s[4], s[5]}, {s[6], s[7]}};
  const cf Rr[4] = {csub(XZ[0], conjf2(XZ[0])), csub(XZ[1], conjf2(XZ[2])),
                    csub(XZ[2], conjf2(XZ[1])), csub(XZ[3], conjf2(XZ[3]))};
  const float l1 = eig[0], l2 = eig[1];
  const cf* Ul = reinterpret_cast<const cf*>(eig + 2);
  const cf U[4] = {Ul[0], Ul[1], Ul[2], Ul[3]};
  cf T[4], Rp[4], Om[4];
  m2hmul(U, Rr, T);
  m2mul(T, U, Rp);
  const float d00 = 1.f / fmaxf(l1 + l1, 1e-30f);
  const float d01 = 1.f / fmaxf(l1 + l2, 1e-30f);
  const float d11 = 1.f / fmaxf(l2 + l2, 1e-30f);
  Rp[0] = cscale(Rp[0], d00); Rp[1] = cscale(Rp[1], d01);
  Rp[2] = cscale(Rp[2], d01); Rp[3] = cscale(Rp[3], d11);
  m2mul(U, Rp, T);
  m2mulh(T, U, Om);
  const cf o0 = csub(z0, cadd(cmul(x0, Om[0]), cmul(x1, Om[2])));
  const cf o1 = csub(z1, cadd(cmul(x0, Om[1]), cmul(x1, Om[3])));
  return make_float4(o0.x, o0.y, o1.x, o1.y);
}

__device__ __forceinline__ void rtr_tcg_body(
    const float* __restrict__ JtJ, const float* __restrict__ Jtr,
    const cf* __restrict__ J, const float* __restrict__ iw,
    const float* __restrict__ delta_, int N, int maxit, float kappa,
    cf* __restrict__ g_out, cf* __restrict__ eta_out, cf* __restrict__ He_out,
    float* __restrict__ stats) {
  extern __shared__ float4 rt_lds[];
  __shared__ float red[RT_NW * RT_RED];
  __shared__ float eig[10];
  const int P = 8 * N, nq = 2 * N;
  float* vb = reinterpret_cast<float*>(rt_lds);   // [P] v of the matvec
  float* hb = vb + P;                             // [P] its result
  float* iws = hb + P;                            // [N]
  const int c = blockIdx.x, tid = threadIdx.x;
  const bool own = tid < nq;
  const size_t q = (size_t)c * nq + tid;          // this thread's quad
  const float* A = JtJ + (size_t)c * P * P;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 x = own ? reinterpret_cast<const float4*>(J)[q] : zero;
  for (int i = tid; i < N; i += RT_TB) iws[i] = iw[i];

  {  // S = X^H X and its eigendecomposition, once
    const cf x0 = {x.x, x.y}, x1 = {x.z, x.w}, s01 = cmulc(x1, x0);
    float s[4] = {cabs2(x0), cabs2(x1), s01.x, s01.y};
    rt_reduce(s, red);
    if (tid == 0) rt_herm2_eig(s[0], s[1], cf{s[2], s[3]}, eig);
    __syncthreads();                              // eig, and iws above
  }

  float4 g = zero;
  if (own) {
    const float4 t = reinterpret_cast<const float4*>(Jtr)[q];
    const float w = iws[tid >> 1];
    g = make_float4((-2.f * t.x) * w, (-2.f * t.y) * w, (-2.f * t.z) * w,
                    (-2.f * t.w) * w);
  }
  g = rt_proj(g, x, eig, red);
  float4 r = g, d = make_float4(-g.x, -g.y, -g.z, -g.w), eta = zero;
  float gg[1] = {rt_dot(g, g)};
  rt_reduce(gg, red);
  gg[0] *= 2.f;
  float r0 = gg[0];
  const float rnorm0 = sqrtf(r0), tol = rnorm0 * fminf(rnorm0, kappa);
  const float delta = delta_[c];
  int nit = 0;
  bool done = false;
  for (int it = 0; it < maxit && !done; ++it) {
    ++nit;
    if (own) reinterpret_cast<float4*>(vb)[tid] = d;
    __syncthreads();
    rt_matvec(A, vb, hb, iws, P);
    __syncthreads();
    const float4 Hd =
        rt_proj(own ? reinterpret_cast<const float4*>(hb)[tid] : zero, x, eig,
                red);
    float s[4] = {rt_dot(d, Hd), rt_dot(eta, eta), rt_dot(eta, d),
                  rt_dot(d, d)};
    rt_reduce(s, red);
    const float dHd = 2.f * s[0], ee = 2.f * s[1], ed = 2.f * s[2],
                dd = 2.f * s[3];
    const float alpha = r0 / fmaxf(dHd, 1e-30f);
    const float4 eta_new = rt_axpy(eta, alpha, d);
    float en[1] = {rt_dot(eta_new, eta_new)};
    rt_reduce(en, red);
    const bool hit = dHd <= 0.f || sqrtf(2.f * en[0]) > delta;
    const float tau =
        (-ed + sqrtf(fmaxf(ed * ed + dd * (delta * delta - ee), 0.f))) /
        fmaxf(dd, 1e-30f);
    eta = hit ? rt_axpy(eta, tau, d) : eta_new;
    done = hit;
    r = rt_axpy(r, alpha, Hd);
    float rn[1] = {rt_dot(r, r)};
    rt_reduce(rn, red);
    rn[0] *= 2.f;
    done = done || sqrtf(rn[0]) <= tol;
    const float beta = rn[0] / fmaxf(r0, 1e-30f);
    d = make_float4(-r.x + beta * d.x, -r.y + beta * d.y, -r.z + beta * d.z,
                    -r.w + beta * d.w);
    r0 = rn[0];
  }
  // Heta = hess_vec(eta), for the model decrease of the outer iteration
  if (own) reinterpret_cast<float4*>(vb)[tid] = eta;
  __syncthreads();
  rt_matvec(A, vb, hb, iws, P);
  __syncthreads();
  const float4 He = rt_proj(
      own ? reinterpret_cast<const float4*>(hb)[tid] : zero, x, eig, red);
  float s[2] = {rt_dot(g, eta), rt_dot(eta, He)};
  rt_reduce(s, red);
  if (own) {
    reinterpret_cast<float4*>(g_out)[q] = g;
    reinterpret_cast<float4*>(eta_out)[q] = eta;
    reinterpret_cast<float4*>(He_out)[q] = He;
  }
  if (tid == 0)
    reinterpret_cast<float4*>(stats)[c] =
        make_float4(gg[0], 2.f * s[0], 2.f * s[1], (float)nit);
}

RT_KERNEL __launch_bounds__(RT_TB)
k_rtr_tcg(RtrTcgArgs a, float2* g, float2* eta, float2* Heta, float* stats) {
  rtr_tcg_body(a.JtJ, a.Jtr, a.J, a.iw, a.delta, a.N, a.maxit, a.kappa, g, eta,
               Heta, stats);
}
