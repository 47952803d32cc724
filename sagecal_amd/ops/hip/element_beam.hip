// Dipole element pattern (E-Jones) of D directions at F frequencies in one
// launch: the producer of the ejones buffer of k_predict_coh_ej /
// k_shapelet_coh_ej (kernel_element_beam role with wideband = 1,
// predict_model.cu:366; eval_elementcoeffs, elementbeam.c:384), in the
// Laguerre-Gaussian basis of beams.LofarElementCoeffs:
//   f_nm(r, t) = P_nm (pi/4 + r)^|m| L_{(n-|m|)/2}^{|m|}(r^2 / beta^2)
//                exp(-r^2 / (2 beta^2)) exp(-j m t),   n < M, m = -n..n by 2
//   E[f,d] = [[sum_i bx_i ct_fi, sum_i bx_i cp_fi],
//             [sum_i by_i ct_fi, sum_i by_i cp_fi]]
// with r = pi/2 - el the zenith angle, bx the mode stack at t = az - pi/4 (X
// dipole), by the stack at t = az + pi/4 (Y dipole), and ct, cp the theta and
// phi coefficient rows of frequency f, which the host has already clamped and
// interpolated. el < 0, decided in fp64, gives four exact zeros.
//
// Work split. One thread owns one direction and builds its Nmodes basis
// values once, in registers: the radial part is shared by +m and -m and by
// both dipoles, exp(-j m t) comes from one sincosf as powers of exp(-j t).
// The Y stack is the X stack times (-j)^m, which depends on m mod 4 alone, so
// per channel the thread sums bx_i ct_fi and bx_i cp_fi into four classes by
// m mod 4 (8 FMAs per mode, not 16); X is s0 + s1 + s2 + s3 and Y is
// s0 - j s1 - s2 + j s3. M is a run-time value: the loops are unrolled to
// the cap EB_MAX_M so every register-array index and class is a constant,
// and tests on the block-uniform M leave them early. A class sum runs in
// mode order whatever F is, so a channel's result does not depend on what
// shares the launch, and repeats bit for bit.
//
// Block size 64, one wave: D is 1e3..1e5 (timeslots x sources), at most a few
// waves per SIMD, so one wave per workgroup spreads them over the most CUs
// and the barriers synchronise nothing but the wave itself. Each wave stages
// its own coefficients, F * Nmodes * 16 B from L2 against F * Nmodes * 8 * 64
// FMAs of use. hipcc reports 172 VGPRs and no scratch (2 waves per SIMD):
// the basis is 72 floats and is kept as operand pairs of packed FMAs.
//
// Chunk EB_NF = 16 channels: 16 * 36 * 16 B = 9 KiB of LDS whatever F is,
// which never limits occupancy before the registers do. Theta and phi of a
// mode are interleaved as one float4 that all lanes read at one address
// (broadcast ds_read_b128, 4 LDS cycles against the 8 FMAs it feeds).
// Staging a chunk is 7 float4 stores per thread against 16 * 28 * 8 FMAs, so
// a larger chunk buys nothing.
//
// Precision: t = az - pi/4 is formed in fp64 and split into a float head and
// tail; sincosf of the head is corrected by the tail to first order, so the
// rounding of t (2.4e-7 at |t| ~ pi, times m in mode m) does not reach the
// result. r is rounded to float once; the rest is fp32.
#define EB_MAX_M ELEMENT_BEAM_MAX_M     // launchers.h: 8, Nmodes <= 36
#define EB_MAX_MODES (EB_MAX_M * (EB_MAX_M + 1) / 2)
#define EB_NF 16
#define EB_TB 64

// From the four class sums s[k] = sum over the modes with m = k mod 4 of
// bx_i c_i: the X-dipole sum, and the Y-dipole sum sum_k (-j)^k s[k]
__device__ __forceinline__ cf eb_xsum(const cf (&s)[4]) {
  return cadd(cadd(s[0], s[2]), cadd(s[1], s[3]));
}
__device__ __forceinline__ cf eb_ysum(const cf (&s)[4]) {
  const cf e = csub(s[0], s[2]), o = csub(s[1], s[3]);   // e + (-j) o
  return {e.x + o.y, e.y - o.x};
}

// acc += b * c
__device__ __forceinline__ void eb_cfma(cf& acc, cf b, float cx, float cy) {
  acc.x = fmaf(b.x, cx, acc.x);
  acc.x = fmaf(-b.y, cy, acc.x);
  acc.y = fmaf(b.x, cy, acc.y);
  acc.y = fmaf(b.y, cx, acc.y);
}

extern "C" __global__ void __launch_bounds__(EB_TB)
k_element_beam(const double* __restrict__ az,       // [D]
               const double* __restrict__ el,       // [D]
               const cf* __restrict__ coef,         // [F, 2, Nmodes]
               const float* __restrict__ preamble,  // [Nmodes]
               int D, int F, int M, float beta,
               cf* __restrict__ E) {                // [F, D, 2, 2]
  __shared__ float4 cs[EB_NF * EB_MAX_MODES];
  const int Nmodes = M * (M + 1) / 2;
  const int d = blockIdx.x * EB_TB + threadIdx.x;
  const bool live = d < D;
  double a = 0.0, e = 0.0;
  if (live) {
    a = az[d];
    e = el[d];
  }
  const bool dark = e < 0.0;       // fp64: a rounded el cannot flip it
  if (dark) e = 0.0;
  const double PI = 3.14159265358979323846;
  const double t = a - 0.25 * PI;
  const float th = (float)t, tl = (float)(t - (double)th);
  float s, c;
  sincosf(th, &s, &c);
  // e1 = exp(-j t), head corrected by the tail
  const cf e1 = {fmaf(-s, tl, c), -fmaf(c, tl, s)};
  const float r = (float)(0.5 * PI - e);
  const float rs = r / beta;
  const float rb = rs * rs;
  const float ex = expf(-0.5f * rb);
  const float base = (float)(0.25 * PI) + r;

  // b[i], i = n(n+1)/2 + (m+n)/2: the X-dipole mode stack. Walk q = |m|, and
  // for each q the Laguerre recurrence in p (n = q + 2p), as
  // LofarElementCoeffs.basis does.
  cf b[EB_MAX_MODES];
  float pw = 1.f;                  // (pi/4 + r)^q
  cf eq = {1.f, 0.f};              // exp(-j q t)
#pragma unroll
  for (int q = 0; q < EB_MAX_M; ++q) {
    if (q < M) {
      const float g = pw * ex;
      float Lp2 = 1.f, Lp1 = 1.f - rb + (float)q;
#pragma unroll
      for (int p = 0; q + 2 * p < EB_MAX_M; ++p) {
        const int n = q + 2 * p;
        if (n < M) {
          float L = p == 0 ? Lp2 : Lp1;
          if (p >= 2) {
            const float p1 = 1.f / (float)p;
            L = (2.f + p1 * ((float)(q - 1) - rb)) * Lp1
                - (1.f + p1 * (float)(q - 1)) * Lp2;
            Lp2 = Lp1;
            Lp1 = L;
          }
          const int ip = n * (n + 1) / 2 + (n + q) / 2;   // m = +q
          const float R = preamble[ip] * (g * L);
          b[ip] = {R * eq.x, R * eq.y};
          if (q > 0) {
            const int im = n * (n + 1) / 2 + (n - q) / 2;  // m = -q
            b[im] = {R * eq.x, -R * eq.y};
          }
        }
      }
      pw *= base;
      eq = cmul(eq, e1);
    }
  }

  for (int f0 = 0; f0 < F; f0 += EB_NF) {
    const int nf = min(EB_NF, F - f0);
    __syncthreads();
#pragma clang loop vectorize(disable) unroll(disable)
    for (int i = threadIdx.x; i < nf * Nmodes; i += EB_TB) {
      const int f = i / Nmodes, k = i - f * Nmodes;
      const cf* row = coef + (size_t)(f0 + f) * 2 * Nmodes;
      const cf ct = row[k], cp = row[Nmodes + k];
      cs[i] = make_float4(ct.x, ct.y, cp.x, cp.y);
    }
    __syncthreads();
#pragma unroll 1
    for (int f = 0; f < nf; ++f) {
      const float4* cm = cs + f * Nmodes;
      // st[k], sp[k]: the theta and phi sums over the modes with m = k mod 4
      cf st[4], sp[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) st[k] = sp[k] = {0.f, 0.f};
#pragma unroll
      for (int n = 0; n < EB_MAX_M; ++n) {
        if (n < M) {
#pragma unroll
          for (int j = 0; j <= n; ++j) {
            const int i = n * (n + 1) / 2 + j;
            const float4 c4 = cm[i];
            eb_cfma(st[(2 * j - n) & 3], b[i], c4.x, c4.y);
            eb_cfma(sp[(2 * j - n) & 3], b[i], c4.z, c4.w);
          }
        }
      }
      const cf xt = eb_xsum(st), xp = eb_xsum(sp);
      const cf yt = eb_ysum(st), yp = eb_ysum(sp);
      if (live) {
        float4* o = reinterpret_cast<float4*>(
            E + ((size_t)(f0 + f) * D + d) * 4);
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        o[0] = dark ? z : make_float4(xt.x, xt.y, xp.x, xp.y);
        o[1] = dark ? z : make_float4(yt.x, yt.y, yp.x, yp.y);
      }
    }
  }
}
