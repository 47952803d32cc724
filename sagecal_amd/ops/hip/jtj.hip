// JtJ / Jtr assembly and model/cost kernels for gfx950 (MI355X).
//
// Replaces the reference's dense-Jacobian path (kernel_jacf mderiv.cu:1069
// + cublasSgemm JtJ in clmfit_cuda.c:364) with direct per-baseline
// closed-form assembly: each baseline contributes 2x2-complex Gram blocks
// (derivation in sagecal_amd/ops/reference.py jtj_jtr). One wave per
// (station-pair, segment): lanes stride the time axis, accumulate complex
// partials in registers, wave-reduce with 64-lane shuffles, then one lane
// commits everything with plain stores to its own (chunk, pair) slot: the
// cross block, and the two stations' diagonal/gradient/cost partials.
// k_jtj_reduce then sums each station's partials over its pairs in a fixed
// order (store pass + per-destination sum pass), so the result is bitwise
// reproducible from run to run — float atomics sum in arrival order, and
// the LM accept/reject chain amplified that last-bit noise to 1e-3.
//
// Row layout contract (host-verified): rows = seg*(T*Nbase) + t*Nbase + b,
// pair table pairs[b] = (p, q), chunk_tab[seg*T + t] = global chunk id.
#include "common.h"

// warp sum over all 64 lanes
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, WAVE);
  return x;
}

// Per-(chunk, pair) slot layout (slot = c*npair_slots + b):
//  Pg  [slots][8]  cf: gradient partials, station p side then q side
//  PD  [slots][8]  cf: diagonal 2x2 block partials, p side then q side
//  Pc  [slots]     float: cost partial
//  Cx  [slots][16] cf: cross block (i,j)x(k,b) complex entries
//  present[Mt] int: set for every chunk this launch covers
extern "C" __global__ void __launch_bounds__(64)
k_jtj_accum(const float2* __restrict__ x, const float2* __restrict__ coh,
            const float2* __restrict__ J,    // [Mt*N*4]
            const int* __restrict__ pairs,   // [Nbase*2]
            const int* __restrict__ chunk_tab,  // [nseg*T]
            const float* __restrict__ wts,   // [B] or nullptr
            int Nbase, int T, int N,
            float2* __restrict__ PD, float2* __restrict__ Pg,
            float2* __restrict__ Cx, float* __restrict__ Pc,
            int* __restrict__ present, int npair_slots, int grad_only) {
  const int b = blockIdx.x;        // pair index
  const int seg = blockIdx.y;
  const int lane = threadIdx.x;
  const int p = pairs[2 * b], q = pairs[2 * b + 1];
  if (p < 0 || q < 0) return;      // flagged pair

  const size_t seg_row0 = (size_t)seg * T * Nbase;

  int t0 = 0;
  while (t0 < T) {
    const int c = chunk_tab[seg * T + t0];   // global chunk id
    // chunk extent [t0, t1)
    int t1 = t0 + 1;
    while (t1 < T && chunk_tab[seg * T + t1] == c) ++t1;

    cf Ap[4] = {}, Aq[4] = {}, gp[4] = {}, gq[4] = {}, Xc[16] = {};
    float cst = 0.f;
    cf J1[4], J2[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      J1[i] = J[((size_t)c * N + p) * 4 + i];
      J2[i] = J[((size_t)c * N + q) * 4 + i];
    }
    for (int t = t0 + lane; t < t1; t += WAVE) {
      const size_t r = seg_row0 + (size_t)t * Nbase + b;
      cf C[4], X[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { C[i] = coh[r * 4 + i]; X[i] = x[r * 4 + i]; }
      const float wt = wts ? wts[r] : 1.0f;
      cf G1[4], K[4], V[4], res[4];
      m2mulh(C, J2, G1);      // G1 = C * J2^H
      m2mul(J1, C, K);        // K  = J1 * C
      m2mul(J1, G1, V);       // V  = J1 * G1
#pragma unroll
      for (int i = 0; i < 4; ++i) res[i] = csub(X[i], V[i]);
      cst += wt * (cabs2(res[0]) + cabs2(res[1]) + cabs2(res[2]) + cabs2(res[3]));
      cf t4[4];
      if (!grad_only) {
        // diag: Ap += w*conj(G1 G1^H); Aq += w*conj(K^H K)
        m2mulh(G1, G1, t4);
#pragma unroll
        for (int i = 0; i < 4; ++i) Ap[i] = cadd(Ap[i], cscale(conjf2(t4[i]), wt));
        m2hmul(K, K, t4);
#pragma unroll
        for (int i = 0; i < 4; ++i) Aq[i] = cadd(Aq[i], cscale(conjf2(t4[i]), wt));
      }
      // grads: gp += w*(res G1^H); gq += w*(res^H K)
      m2mulh(res, G1, t4);
#pragma unroll
      for (int i = 0; i < 4; ++i) gp[i] = cadd(gp[i], cscale(t4[i], wt));
      m2hmul(res, K, t4);
#pragma unroll
      for (int i = 0; i < 4; ++i) gq[i] = cadd(gq[i], cscale(t4[i], wt));
      // cross: Xc[(i,j),(k,b2)] += w * conj(G1[j,k]) * K[i,b2]
      if (grad_only) continue;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int b2 = 0; b2 < 2; ++b2) {
              cf v2 = cmul(conjf2(G1[2 * j + k]), K[2 * i + b2]);
              int idx = (2 * i + j) * 4 + (2 * k + b2);
              Xc[idx] = cadd(Xc[idx], cscale(v2, wt));
            }
    }
    // wave reduction of all partials
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      gp[i].x = wave_sum(gp[i].x); gp[i].y = wave_sum(gp[i].y);
      gq[i].x = wave_sum(gq[i].x); gq[i].y = wave_sum(gq[i].y);
    }
    if (!grad_only) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        Ap[i].x = wave_sum(Ap[i].x); Ap[i].y = wave_sum(Ap[i].y);
        Aq[i].x = wave_sum(Aq[i].x); Aq[i].y = wave_sum(Aq[i].y);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        Xc[i].x = wave_sum(Xc[i].x); Xc[i].y = wave_sum(Xc[i].y);
      }
    }
    cst = wave_sum(cst);
    if (lane == 0) {
      const size_t slot = (size_t)c * npair_slots + b;   // unique writer
      float2* Gs = Pg + slot * 8;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        Gs[i] = gp[i];
        Gs[4 + i] = gq[i];
      }
      if (!grad_only) {
        float2* Ds = PD + slot * 8;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          Ds[i] = Ap[i];
          Ds[4 + i] = Aq[i];
        }
        float2* Xo = Cx + slot * 16;
#pragma unroll
        for (int i = 0; i < 16; ++i) Xo[i] = Xc[i];
      }
      Pc[slot] = cst;
      present[c] = 1;      // same value from every writer
    }
    t0 = t1;
  }
}

// Sum pass of k_jtj_accum's slots. Block (s, c), s < N: station s of
// chunk c sums its side of every pair it belongs to (lane-strided over the
// partner station, then the fixed 64-lane shuffle tree). Block (N, c):
// the chunk's cost. Chunks the accumulate launch did not cover keep the
// zeros the host put into D/g/cost.
extern "C" __global__ void __launch_bounds__(64)
k_jtj_reduce(const float2* __restrict__ PD, const float2* __restrict__ Pg,
             const float* __restrict__ Pc, const int* __restrict__ present,
             const int* __restrict__ pairs,  // [Nbase*2]
             const int* __restrict__ pidx,   // [N*N] pair index or -1
             int N, int Nbase, int npair_slots, int grad_only,
             float2* __restrict__ D, float2* __restrict__ g,
             float* __restrict__ cost) {
  const int s = blockIdx.x;
  const int c = blockIdx.y;
  const int lane = threadIdx.x;
  if (!present[c]) return;         // uniform over the block
  const size_t slot0 = (size_t)c * npair_slots;
  if (s == N) {
    float cs = 0.f;
    for (int b = lane; b < Nbase; b += WAVE) {
      if (pairs[2 * b] >= 0 && pairs[2 * b + 1] >= 0) cs += Pc[slot0 + b];
    }
    cs = wave_sum(cs);
    if (lane == 0) cost[c] = cs;
    return;
  }
  cf sg[4] = {}, sd[4] = {};
  for (int o = lane; o < N; o += WAVE) {
    if (o == s) continue;
    const int lo = o < s ? o : s, hi = o < s ? s : o;
    const int pi = pidx[lo * N + hi];
    if (pi < 0 || pi >= Nbase) continue;
    int side;
    if (pairs[2 * pi] == s) side = 0;
    else if (pairs[2 * pi + 1] == s) side = 4;
    else continue;                 // pair flagged in this layout
    const float2* a = Pg + (slot0 + pi) * 8 + side;
#pragma unroll
    for (int i = 0; i < 4; ++i) sg[i] = cadd(sg[i], a[i]);
    if (!grad_only) {
      const float2* d = PD + (slot0 + pi) * 8 + side;
#pragma unroll
      for (int i = 0; i < 4; ++i) sd[i] = cadd(sd[i], d[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    sg[i].x = wave_sum(sg[i].x); sg[i].y = wave_sum(sg[i].y);
    if (!grad_only) {
      sd[i].x = wave_sum(sd[i].x); sd[i].y = wave_sum(sd[i].y);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      g[((size_t)c * N + s) * 4 + i] = sg[i];
      if (!grad_only) D[((size_t)c * N + s) * 4 + i] = sd[i];
    }
  }
}

// Expand accumulators into the dense JtJ [Mt, 8N, 8N] + Jtr [Mt, 8N].
// One 64-thread block per (chunk, s1, s2) 8x8 block; thread per entry.
// k_jtj_accum stored the cross block of pair pi with rows = parameters of
// station pairs[2*pi] and columns = those of pairs[2*pi+1], whichever of
// the two has the lower number: block (s1, s2) takes it as stored when s1
// is the pair's first station and transposed when it is the second.
extern "C" __global__ void __launch_bounds__(64)
k_jtj_expand(const float2* __restrict__ D, const float2* __restrict__ g,
             const float2* __restrict__ Cx,
             const int* __restrict__ pairs,  // [npair_slots*2]
             const int* __restrict__ pidx,   // [N*N] pair index or -1
             int N, int npair_slots,
             float* __restrict__ JtJ, float* __restrict__ Jtr) {
  const int c = blockIdx.z;
  const int s1 = blockIdx.y;
  const int s2 = blockIdx.x;
  const int e = threadIdx.x;        // 0..63 entry in 8x8 block
  const int row = e >> 3, col = e & 7;
  const size_t P = (size_t)8 * N;
  float val = 0.f;
  if (s1 == s2) {
    // I2 (x) realify(A): block diag 4x4 repeated. A is Hermitian only to
    // rounding (its diagonal carries an imaginary residue, A[1] is not
    // bitwise conj(A[2])), so the entries above the diagonal mirror the
    // ones below, which the Cholesky kernels read: JtJ == JtJ^T exactly
    if ((row >> 2) == (col >> 2)) {
      const cf* A = D + ((size_t)c * N + s1) * 4;
      const int r4 = max(row, col) & 3, c4 = min(row, col) & 3;
      const cf a = A[(r4 >> 1) * 2 + (c4 >> 1)];
      // realify: [[ar,-ai],[ai,ar]]
      val = ((r4 & 1) == 0) ? (((c4 & 1) == 0) ? a.x : -a.y)
                            : (((c4 & 1) == 0) ? a.y : a.x);
    }
    if (e < 8) {
      // Jtr entry: vecR of g (row-major interleaved re/im)
      const cf* G = g + ((size_t)c * N + s1) * 4;
      const cf gv = G[e >> 1];
      Jtr[(size_t)c * P + 8 * s1 + e] = (e & 1) ? gv.y : gv.x;
    }
  } else {
    const int lo = min(s1, s2), hi = max(s1, s2);
    const int pi = pidx[lo * N + hi];
    if (pi >= 0 && pi < npair_slots) {
      const int first = pairs[2 * pi], second = pairs[2 * pi + 1];
      // a pair flagged in this layout (or a table of another layout)
      // names neither station: the block stays zero
      if ((first == s1 && second == s2) || (first == s2 && second == s1)) {
        const cf* X = Cx + ((size_t)c * npair_slots + pi) * 16;
        // antirealify: entry ((ij),(kb)) complex v -> [[vx,vy],[vy,-vx]]
        int rr = row, cc = col;
        if (first != s1) { rr = col; cc = row; }   // transpose block
        const cf v2 = X[(rr >> 1) * 4 + (cc >> 1)];
        val = ((rr & 1) == 0) ? (((cc & 1) == 0) ? v2.x : v2.y)
                              : (((cc & 1) == 0) ? v2.y : -v2.x);
      }
    }
  }
  JtJ[(size_t)c * P * P + ((size_t)8 * s1 + row) * P + 8 * s2 + col] = val;
}

// Per-row weighted model cost e2[r] = w*|x - J1 C J2^H|^2 (0 for flagged
// pairs); k_slot_cost and k_chunk_cost sum the rows of each chunk in a
// fixed order, so the per-chunk cost is reproducible (no float atomics).
extern "C" __global__ void __launch_bounds__(256)
k_model_cost(const float2* __restrict__ x, const float2* __restrict__ coh,
             const float2* __restrict__ J,
             const int* __restrict__ pairs,
             const int* __restrict__ chunk_tab,
             const float* __restrict__ wts,
             int Nbase, int T, int N, int nseg,
             float* __restrict__ e2) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t B = (size_t)nseg * T * Nbase;
  float cst = 0.f;
  if (r < B) {
    const int b = (int)(r % Nbase);
    const int st = (int)(r / Nbase);     // seg*T + t
    const int c = chunk_tab[st];
    const int p = pairs[2 * b], q = pairs[2 * b + 1];
    if (p >= 0) {
      cf J1[4], J2[4], C[4], G1[4], V[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        J1[i] = J[((size_t)c * N + p) * 4 + i];
        J2[i] = J[((size_t)c * N + q) * 4 + i];
        C[i] = coh[r * 4 + i];
      }
      m2mulh(C, J2, G1);
      m2mul(J1, G1, V);
      const float wt = wts ? wts[r] : 1.0f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        cf d = csub(x[r * 4 + i], V[i]);
        cst += wt * cabs2(d);
      }
    }
    e2[r] = cst;
  }
}

// fixed-order sum of one value per thread over a 256-thread block
__device__ __forceinline__ float block_sum256(float s) {
  __shared__ float ws[256 / WAVE];
  const int tid = threadIdx.x;
  s = wave_sum(s);
  if ((tid & (WAVE - 1)) == 0) ws[tid / WAVE] = s;
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int i = 0; i < 256 / WAVE; ++i) tot += ws[i];
  return tot;
}

// slot_cost[st] = sum of e2 over the Nbase rows of (seg, t) slot st: one
// block per slot, threads stride the rows.
extern "C" __global__ void __launch_bounds__(256)
k_slot_cost(const float* __restrict__ e2, int Nbase,
            float* __restrict__ slot_cost) {
  const int st = blockIdx.x;
  const float* row = e2 + (size_t)st * Nbase;
  float s = 0.f;
  for (int b = threadIdx.x; b < Nbase; b += 256) s += row[b];
  s = block_sum256(s);
  if (threadIdx.x == 0) slot_cost[st] = s;
}

// cost[c] = sum of slot_cost over the slots of chunk c: one block per
// chunk, threads stride the slot table (independent loads, no serial
// scan), other chunks' slots contribute 0.
extern "C" __global__ void __launch_bounds__(256)
k_chunk_cost(const float* __restrict__ slot_cost,
             const int* __restrict__ chunk_tab, int nslots,
             float* __restrict__ cost) {
  const int c = blockIdx.x;
  float s = 0.f;
  for (int st = threadIdx.x; st < nslots; st += 256) {
    if (chunk_tab[st] == c) s += slot_cost[st];
  }
  s = block_sum256(s);
  if (threadIdx.x == 0) cost[c] = s;
}

// Model application: V[r] (sub=0) or residual x - sum_ci V (sub=1).
// cohs: [M, R, 4]; chunk_tab per cluster: [M, nseg*T].
extern "C" __global__ void __launch_bounds__(256)
k_apply_jones(const float2* __restrict__ x,      // may be null when sub=0
              const float2* __restrict__ cohs,
              const float2* __restrict__ J,
              const int* __restrict__ pairs,
              const int* __restrict__ chunk_tab,  // [M * nseg*T]
              int Nbase, int T, int N, int nseg, int M, int sub,
              float2* __restrict__ out) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t B = (size_t)nseg * T * Nbase;
  if (r >= B) return;
  const int b = (int)(r % Nbase);
  const int st = (int)(r / Nbase);
  const int p = pairs[2 * b], q = pairs[2 * b + 1];
  cf acc[4] = {};
  if (p >= 0) {
    for (int ci = 0; ci < M; ++ci) {
      const int c = chunk_tab[(size_t)ci * nseg * T + st];
      cf J1[4], J2[4], C[4], G1[4], V[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        J1[i] = J[((size_t)c * N + p) * 4 + i];
        J2[i] = J[((size_t)c * N + q) * 4 + i];
        C[i] = cohs[((size_t)ci * B + r) * 4 + i];
      }
      m2mulh(C, J2, G1);
      m2mul(J1, G1, V);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = cadd(acc[i], V[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    cf o = acc[i];
    if (sub) o = csub(x[r * 4 + i], o);
    out[r * 4 + i] = o;
  }
}
