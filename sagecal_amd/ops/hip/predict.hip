// Coherency predict kernel for gfx950 (MI355X).
//
// MI355X-native replacement for the reference's kernel_coherencies
// (predict_model.cu:1059): one thread per baseline-row, sources staged
// through LDS in tiles, fp64 phase arithmetic with double-precision arg
// reduction followed by fast float sincos. Per-channel fluxes are
// precomputed on the host (torch), so the kernel carries no spectral-index
// math. Shapelet sources have their fluxes zeroed for k_predict_coh and
// are added by k_shapelet_coh (below), launched after it on the same
// stream from a device-resident mode table (hip_host.ShapeletTable).
//
// Layout: rows r = t*Nbase + b (time-major); output coh [M, R, 4] complex64.
//
// Optional fused station-beam path (-B 1, the reference's DOBEAM_ARRAY:
// predict_model.cu:843-852 'scalef *= beam1*beam2'): when `beam` is
// non-null it holds the REAL scalar array-factor gain per
// (timeslot, source, station) [T, K, N] (beamgain = |sum phasors|/K,
// stationbeam.c:318 — the reference's array factor is real), and each
// source's contribution is scaled by beam[t,g,sta1]*beam[t,g,sta2].
//
// Optional element-beam path (-B 2/3, DOBEAM_FULL / DOBEAM_ELEMENT,
// predict_model.cu:843-852 with elementgain): the _ej kernels take the
// dipole E-Jones per (timeslot, source, pattern) [T, K, NE, 2, 2]
// complex64, NE = 1 (one pattern per array origin) or Nsta, and add
// g_p g_q E_p C E_q^H per source. The sandwich differs per source, so the
// accumulators are the four coherency entries instead of four Stokes sums.
// They are compile-time variants (template parameter EJ) of one body: the
// kernels without E-Jones carry none of this code and no branch for it.
//
// Arguments. The kernels take the structs of launchers.h by value (RowsUVW,
// SourceArrays or ShapeletTab, Channel, BeamArgs), the same ones the
// bindings fill by field name. Each kernel family has one unpack function
// (predict_coh_kernel, shapelet_coh_kernel) that forwards the fields to the
// __restrict__ parameter list of a __device__ __forceinline__ body, and
// bodies and helpers work on those parameters and on values only, never on
// a struct member. __restrict__ carries noalias on function parameters
// alone: through a struct member, or a local __restrict__ copy of one, the
// compiler cannot prove that the out[] read-modify-write of k_shapelet_coh
// leaves the table alone, and turns the block-uniform table reads from
// scalar into per-lane vector loads. hipcc -O3 for gfx950, k_shapelet_coh
// (the _ej kernel moves the same way, 748/69/48/14 -> 760/73/18/42):
//                                       instrs  VGPR  s_load  global_load
//   positional arguments                   632    50      47           10
//   body reads struct members              642    52      15           38
//   struct fields forwarded to the body    628    50      43           10
// (this file as it stands: 629/50/43/10 and 738/69/46/14). Two more things
// cost VGPRs in the _ej kernels, so the helpers avoid them: a second local
// array between the sums and the store (put_coherency hands each entry to
// a callback), and fluxes read before the beam gains (add_source takes a
// flux(i) callable).
#include "common.h"
#include "launchers.h"

#define SRC_TILE 64

struct SrcTile {
  double ll[SRC_TILE], mm[SRC_TILE], nn1[SRC_TILE];
  float flux[4][SRC_TILE];  // Stokes I,Q,U,V
  float eX[SRC_TILE], eY[SRC_TILE], eP[SRC_TILE];
  float cxi[SRC_TILE], sxi[SRC_TILE], cphi[SRC_TILE], sphi[SRC_TILE];
  float r1[SRC_TILE];  // time-smear source-distance term (precomputed host)
  int   stype[SRC_TILE];
};

// cos/sin of an fp64 phase: argument reduced in fp64, then the fast float
// sincos. Shared by phase_smear and k_array_beam.
__device__ __forceinline__ void sincos_reduced(double ph, float* sp,
                                               float* cp) {
  const float phr = (float)fmod(ph, 6.283185307179586476925286766559);
  __sincosf(phr, sp, cp);
}

// The pieces of phase_smear. Only the phase and the time smearing depend
// on the channel; the all-channels kernels (predict_mf.hip) take the other
// two once per source and row.
// fp64 phase term G = 2*pi*(u l + v m + w (n-1)) (seconds * none)
__device__ __forceinline__ double phase_term(double ur, double vr, double wr,
                                             double l, double m, double n1) {
  return 6.283185307179586476925286766559 * (ur * l + vr * m + wr * n1);
}

// freq smearing |sinc(G*fdelta/2)| (predict.c:178-189)
__device__ __forceinline__ float freq_smear(double G, double fdelta2) {
  float sm = 1.0f;
  const float smf = (float)(G * fdelta2);
  if (fabsf(smf) > 1e-9f) sm = fabsf(__sinf(smf) / smf);
  return sm;
}

// sm times the time smearing (predict.c:94-107); r1 precomputed per source
__device__ __forceinline__ float time_smear(float sm, float tsm_c, float r1) {
  const float prod = tsm_c * r1;
  if (prod > 1e-9f) sm *= 1.0645f * erff(0.8326f * prod) / prod;
  return sm;
}

// Smeared phase term of one source at one row, shared by k_predict_coh and
// k_shapelet_coh: exp(i*phase) * freq smearing * time smearing.
__device__ __forceinline__ cf phase_smear(double ur, double vr, double wr,
                                          double l, double m, double n1,
                                          double freq, double fdelta2,
                                          float tsm_c, float r1) {
  const double G = phase_term(ur, vr, wr, l, m, n1);
  // phase at this channel, arg-reduced in fp64 then fast float sincos
  const double ph = fma(G, freq, 0.0);
  float sp, cp;
  sincos_reduced(ph, &sp, &cp);
  const float sm = time_smear(freq_smear(G, fdelta2), tsm_c, r1);
  return {cp * sm, sp * sm};
}

// acc += g * E_p * (phc * [[I+Q, U+iV],[U-iV, I-Q]]) * E_q^H, the
// contribution of one source to the four coherency entries of one row.
// ep, eq: row-major 2x2 complex.
__device__ __forceinline__ void ej_accumulate(cf phc, float fI, float fQ,
                                              float fU, float fV, float g,
                                              const cf* ep, const cf* eq,
                                              cf* acc) {
  const cf E[4] = {ep[0], ep[1], ep[2], ep[3]};
  const cf F[4] = {eq[0], eq[1], eq[2], eq[3]};
  phc = cscale(phc, g);
  const cf C[4] = {cscale(phc, fI + fQ), cmul(phc, {fU, fV}),
                   cmul(phc, {fU, -fV}), cscale(phc, fI - fQ)};
  cf EC[4], S[4];
  m2mul(E, C, EC);
  m2mulh(EC, F, S);
  for (int i = 0; i < 4; ++i) acc[i] = cadd(acc[i], S[i]);
}

// Beam indexing state of one row: its two stations, their E-Jones patterns
// and the offset of its timeslot in units of sources.
struct BeamRow {
  int sta1, sta2;    // stations of the baseline (index into beam[t,k,:])
  int pat1, pat2;    // E-Jones pattern of each: its own, or 0 when NE == 1
  size_t toff;       // t * Ktot
};

// `on`: the row is live and there is a beam or E-Jones; all zero otherwise,
// and pairs is not read.
__device__ __forceinline__ BeamRow beam_row(bool on, int r,
                                            const int* __restrict__ pairs,
                                            int Nbase, int Ktot, int NE) {
  BeamRow br = {0, 0, 0, 0, 0};
  if (on) {
    const int t = r / Nbase, bl = r - t * Nbase;
    br.sta1 = pairs[2 * bl];
    br.sta2 = pairs[2 * bl + 1];
    br.toff = (size_t)t * Ktot;
  }
  br.pat1 = NE == 1 ? 0 : br.sta1;
  br.pat2 = NE == 1 ? 0 : br.sta2;
  return br;
}

// Adds source `src` (index along K) with phase term phc to the sums of one
// row, scaled by the beam gains of the row's stations when beam is
// non-null. flux(i), i = 0..3, reads its Stokes I,Q,U,V; it is called after
// the beam lookup, the order the kernels' register budget was tuned with.
// The sums a[4] are the Stokes sums I,Q,U,V of phc*flux, or with EJ the
// four coherency entries after the sandwich.
template <bool EJ, typename Flux>
__device__ __forceinline__ void add_source(
    cf phc, Flux flux, int src, const BeamRow& br,
    const float* __restrict__ beam, int Nsta,
    const float2* __restrict__ ejones, int NE, cf* a) {
  if constexpr (EJ) {
    const size_t tk = br.toff + (size_t)src;
    float g = 1.0f;
    if (beam != nullptr) {
      const float* bg = beam + tk * (size_t)Nsta;
      g = bg[br.sta1] * bg[br.sta2];
    }
    const cf* ej = ejones + tk * (size_t)NE * 4;
    ej_accumulate(phc, flux(0), flux(1), flux(2), flux(3), g,
                  ej + 4 * br.pat1, ej + 4 * br.pat2, a);
  } else {
    if (beam != nullptr) {
      const float* bg = beam + (br.toff + (size_t)src) * (size_t)Nsta;
      phc = cscale(phc, bg[br.sta1] * bg[br.sta2]);
    }
    for (int i = 0; i < 4; ++i) a[i] = cadd(a[i], cscale(phc, flux(i)));
  }
}

// Hands put(i, c) the four coherency entries of the sums a[4] of
// add_source: with EJ the sums themselves, else Stokes -> coherency
// [[I+Q, U+jV],[U-jV, I-Q]] (predict.c:228-235). k_predict_coh stores them,
// k_shapelet_coh adds them.
template <bool EJ, typename Put>
__device__ __forceinline__ void put_coherency(const cf* a, Put put) {
  if constexpr (EJ) {
    for (int i = 0; i < 4; ++i) put(i, a[i]);
  } else {
    put(0, cadd(a[0], a[1]));
    put(1, {a[2].x - a[3].y, a[2].y + a[3].x});
    put(2, {a[2].x + a[3].y, a[2].y - a[3].x});
    put(3, csub(a[0], a[1]));
  }
}

template <bool EJ>
__device__ __forceinline__ void predict_coh_body(
    const double* __restrict__ u, const double* __restrict__ v,
    const double* __restrict__ w, int R,
    const double* __restrict__ ll, const double* __restrict__ mm,
    const double* __restrict__ nn1,
    const float* __restrict__ sI, const float* __restrict__ sQ,
    const float* __restrict__ sU, const float* __restrict__ sV,
    const float* __restrict__ eX, const float* __restrict__ eY,
    const float* __restrict__ eP, const float* __restrict__ cxi,
    const float* __restrict__ sxi, const float* __restrict__ cphi,
    const float* __restrict__ sphi, const float* __restrict__ r1t,
    const int* __restrict__ stype, const int* __restrict__ cluster_off,
    int M, double freq, double fdelta2, double tdelta,
    const float* __restrict__ beam, const int* __restrict__ pairs,
    int Nbase, int Ktot, int Nsta, const float2* __restrict__ ejones,
    int NE, float2* __restrict__ out) {
  __shared__ SrcTile tile;
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = r < R;
  const BeamRow br = beam_row((EJ || beam != nullptr) && live, r, pairs,
                              Nbase, Ktot, NE);
  double ur = 0, vr = 0, wr = 0;
  float blf = 0.f;
  if (live) {
    ur = u[r]; vr = v[r]; wr = w[r];
    blf = (float)(sqrt(ur * ur + vr * vr + wr * wr) * freq);
  }
  const float uf = (float)(ur * freq), vf = (float)(vr * freq),
              wf = (float)(wr * freq);
  const float tsm_c = 7.2921150e-5f * (float)tdelta * blf;

  for (int ci = 0; ci < M; ++ci) {
    const int s0 = cluster_off[ci], s1 = cluster_off[ci + 1];
    // sums of add_source: IIl/QQl/UUl/VVl as complex, or with EJ the four
    // coherency entries themselves
    cf acc[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
    for (int base = s0; base < s1; base += SRC_TILE) {
      const int nt = min(SRC_TILE, s1 - base);
      __syncthreads();
      for (int k = threadIdx.x; k < nt; k += blockDim.x) {
        const int g = base + k;
        tile.ll[k] = ll[g];   tile.mm[k] = mm[g];   tile.nn1[k] = nn1[g];
        tile.flux[0][k] = sI[g];   tile.flux[1][k] = sQ[g];
        tile.flux[2][k] = sU[g];   tile.flux[3][k] = sV[g];
        tile.eX[k] = eX[g];   tile.eY[k] = eY[g];   tile.eP[k] = eP[g];
        tile.cxi[k] = cxi[g]; tile.sxi[k] = sxi[g];
        tile.cphi[k] = cphi[g]; tile.sphi[k] = sphi[g];
        tile.r1[k] = r1t[g];  tile.stype[k] = stype[g];
      }
      __syncthreads();
      if (!live) continue;
      for (int k = 0; k < nt; ++k) {
        cf phc = phase_smear(ur, vr, wr, tile.ll[k], tile.mm[k], tile.nn1[k],
                             freq, fdelta2, tsm_c, tile.r1[k]);
        // extended-source envelope at wavelength-scaled uvw
        const int st = tile.stype[k];
        if (st != 0) {
          float up = uf, vp = vf;
          // projection rotation (predict.c:36-44); host bakes use_projection
          // into cxi/sxi/cphi/sphi (identity values when off)
          const float c_xi = tile.cxi[k], s_xi = tile.sxi[k];
          const float c_ph = tile.cphi[k], s_ph = tile.sphi[k];
          up = uf * c_xi - vf * c_ph * s_xi + wf * s_ph * s_xi;
          vp = uf * s_xi + vf * c_ph * c_xi - wf * s_ph * c_xi;
          if (st == 1) {  // gaussian
            float cpp, spp;
            __sincosf(tile.eP[k], &spp, &cpp);
            const float ut = tile.eX[k] * (cpp * up - spp * vp);
            const float vt = tile.eY[k] * (spp * up + cpp * vp);
            phc = cscale(phc, __expf(-19.739208802178716f * (ut * ut + vt * vt)));
          } else if (st == 2) {  // disk: j1
            const float b = sqrtf(up * up + vp * vp) * tile.eX[k] *
                            6.2831853071795865f;
            phc = cscale(phc, j1f(b));
          } else if (st == 3) {  // ring: j0
            const float b = sqrtf(up * up + vp * vp) * tile.eX[k] *
                            6.2831853071795865f;
            phc = cscale(phc, j0f(b));
          }
          // st==4 (shapelet): fluxes are zero here, k_shapelet_coh adds them
        }
        add_source<EJ>(phc, [&](int i) { return tile.flux[i][k]; }, base + k,
                       br, beam, Nsta, ejones, NE, acc);
      }
    }
    if (live) {
      float2* o = out + ((size_t)ci * R + r) * 4;
      put_coherency<EJ>(acc, [&](int i, cf c) { o[i] = c; });
    }
    __syncthreads();
  }
}

// The one place that unpacks the argument structs of this kernel family.
// Without EJ the body gets no E-Jones, whatever bm holds.
template <bool EJ>
__device__ __forceinline__ void predict_coh_kernel(
    const RowsUVW& rows, const SourceArrays& s, const Channel& ch,
    const BeamArgs& bm, float2* __restrict__ out) {
  predict_coh_body<EJ>(
      rows.u, rows.v, rows.w, rows.R, s.ll, s.mm, s.nn1, s.sI, s.sQ, s.sU,
      s.sV, s.eX, s.eY, s.eP, s.cxi, s.sxi, s.cphi, s.sphi, s.r1, s.stype,
      s.cluster_off, s.M, ch.freq, ch.fdelta2, ch.tdelta, bm.beam, bm.pairs,
      bm.Nbase, bm.Ktot, bm.Nsta, EJ ? bm.ejones : nullptr, EJ ? bm.NE : 0,
      out);
}

extern "C" __global__ void __launch_bounds__(128)
k_predict_coh(RowsUVW rows, SourceArrays src, Channel ch, BeamArgs bm,
              float2* __restrict__ out) {
  predict_coh_kernel<false>(rows, src, ch, bm, out);
}

// E-Jones variant: pairs, Nbase and Ktot are required; beam may be null.
extern "C" __global__ void __launch_bounds__(128)
k_predict_coh_ej(RowsUVW rows, SourceArrays src, Channel ch, BeamArgs bm,
                 float2* __restrict__ out) {
  predict_coh_kernel<true>(rows, src, ch, bm, out);
}

// Shapelet sources, added into the coherencies k_predict_coh has written
// (launched after it on the same stream; k_predict_coh sees their fluxes
// zeroed). One thread per row; the loop over the S table entries is
// block-uniform, so parameters, coefficients and recurrence constants are
// uniform loads. Entries are sorted by source index (cluster ids
// non-decreasing): Stokes sums stay in registers while the cluster id
// repeats and are added to out[ci, r, :] on a change — each (ci, r)
// belongs to one thread, so the sums need no atomics.
//
// Envelope of entry s at wavelength-scaled (u,v,w) (shapelet.c:141-188):
//   up = psign (u cxi - v cphi sxi + w sphi sxi)   psign = -1 projected,
//   vp = psign (u sxi + v cphi cxi - w sphi cxi)   else +1 with identity
//   ut = a (ceP up - seP vp),  vt = b (seP up + ceP vp)
//   env = sum_{n1,n2} coef[n2 n0 + n1] phi_n1(-ut beta) phi_n2(vt beta)
// taken as real for even n1+n2 and imaginary for odd; the i^(n1+n2) sign
// and 2 pi a b are folded into coef on the host. phi_n is the normalised
// Hermite function, phi_0 = e^{-x^2/2}/sqrt(2), phi_n = x sqrt(2/n)
// phi_{n-1} - sqrt((n-1)/n) phi_{n-2}; rec holds the two constants per n.
template <bool EJ>
__device__ __forceinline__ void shapelet_coh_body(
    const double* __restrict__ u, const double* __restrict__ v,
    const double* __restrict__ w, int R,
    const int* __restrict__ src, const int* __restrict__ cluster,
    const int* __restrict__ n0t, const float* __restrict__ betat,
    const int* __restrict__ off, const float* __restrict__ coef,
    const float* __restrict__ cxi, const float* __restrict__ sxi,
    const float* __restrict__ cphi, const float* __restrict__ sphi,
    const float* __restrict__ psign, const float* __restrict__ at,
    const float* __restrict__ bt, const float* __restrict__ ceP,
    const float* __restrict__ seP, const double* __restrict__ ll,
    const double* __restrict__ mm, const double* __restrict__ nn1,
    const float* __restrict__ rec, int S, int nmax,
    const float* __restrict__ flux, const float* __restrict__ r1t,
    double freq, double fdelta2, double tdelta,
    const float* __restrict__ beam, const int* __restrict__ pairs,
    int Nbase, int Ktot, int Nsta, const float2* __restrict__ ejones,
    int NE, float2* out) {              // [M, R, 4], added into
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const BeamRow br = beam_row(EJ || beam != nullptr, r, pairs, Nbase, Ktot,
                              NE);
  const double ur = u[r], vr = v[r], wr = w[r];
  const float blf = (float)(sqrt(ur * ur + vr * vr + wr * wr) * freq);
  const float uf = (float)(ur * freq), vf = (float)(vr * freq),
              wf = (float)(wr * freq);
  const float tsm_c = 7.2921150e-5f * (float)tdelta * blf;
  const float* rec0 = rec;          // sqrt(2/n)
  const float* rec1 = rec + nmax;   // sqrt((n-1)/n)

  // sums of add_source, as in k_predict_coh
  cf acc[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
  auto flush = [&](int ci) {
    float2* o = out + ((size_t)ci * R + r) * 4;
    put_coherency<EJ>(acc, [&](int i, cf c) { o[i] = cadd(o[i], c); });
  };
  int cur = cluster[0];
  for (int s = 0; s < S; ++s) {
    const int ci = cluster[s];
    if (ci != cur) {
      flush(cur);
      for (int i = 0; i < 4; ++i) acc[i] = {0.f, 0.f};
      cur = ci;
    }
    cf phc = phase_smear(ur, vr, wr, ll[s], mm[s], nn1[s], freq, fdelta2,
                         tsm_c, r1t[s]);
    const float c_xi = cxi[s], s_xi = sxi[s];
    const float c_ph = cphi[s], s_ph = sphi[s];
    const float up = psign[s] *
        (uf * c_xi - vf * c_ph * s_xi + wf * s_ph * s_xi);
    const float vp = psign[s] *
        (uf * s_xi + vf * c_ph * c_xi - wf * s_ph * c_xi);
    const float ut = at[s] * (ceP[s] * up - seP[s] * vp);
    const float vt = bt[s] * (seP[s] * up + ceP[s] * vp);
    const float beta = betat[s];
    const float xu = -ut * beta, xv = vt * beta;
    const float pu0 = 0.70710678118654752f * expf(-0.5f * xu * xu);
    const int n0 = n0t[s];
    const float* cf_s = coef + off[s];
    float re = 0.f, im = 0.f;
    float pv1 = 0.f, pv = 0.70710678118654752f * expf(-0.5f * xv * xv);
    for (int n2 = 0; n2 < n0; ++n2) {
      if (n2 > 0) {
        const float t = xv * rec0[n2] * pv - rec1[n2] * pv1;
        pv1 = pv;
        pv = t;
      }
      // row sums over even and odd n1
      float se = 0.f, so = 0.f;
      float pu1 = 0.f, pu = pu0;
      const float* c = cf_s + n2 * n0;
      for (int n1 = 0; n1 < n0; ++n1) {
        if (n1 > 0) {
          const float t = xu * rec0[n1] * pu - rec1[n1] * pu1;
          pu1 = pu;
          pu = t;
        }
        if (n1 & 1) so += c[n1] * pu;
        else        se += c[n1] * pu;
      }
      if (n2 & 1) { re += pv * so; im += pv * se; }
      else        { re += pv * se; im += pv * so; }
    }
    phc = cmul(phc, {re, im});
    add_source<EJ>(phc, [&](int i) { return flux[i * S + s]; }, src[s], br,
                   beam, Nsta, ejones, NE, acc);
  }
  flush(cur);
}

// The one place that unpacks the argument structs of this kernel family.
template <bool EJ>
__device__ __forceinline__ void shapelet_coh_kernel(
    const RowsUVW& rows, const ShapeletTab& t, const Channel& ch,
    const BeamArgs& bm, float2* out) {
  shapelet_coh_body<EJ>(
      rows.u, rows.v, rows.w, rows.R, t.src, t.cluster, t.n0, t.beta, t.off,
      t.coef, t.cxi, t.sxi, t.cphi, t.sphi, t.psign, t.a, t.b, t.ceP, t.seP,
      t.ll, t.mm, t.nn1, t.rec, t.S, t.nmax, t.flux, t.r1, ch.freq,
      ch.fdelta2, ch.tdelta, bm.beam, bm.pairs, bm.Nbase, bm.Ktot, bm.Nsta,
      EJ ? bm.ejones : nullptr, EJ ? bm.NE : 0, out);
}

extern "C" __global__ void __launch_bounds__(128)
k_shapelet_coh(RowsUVW rows, ShapeletTab tab, Channel ch, BeamArgs bm,
               float2* out) {
  shapelet_coh_kernel<false>(rows, tab, ch, bm, out);
}

// E-Jones variant: E is indexed by the table's source index src[s], like
// the beam; pairs, Nbase and Ktot are required, beam may be null.
extern "C" __global__ void __launch_bounds__(128)
k_shapelet_coh_ej(RowsUVW rows, ShapeletTab tab, Channel ch, BeamArgs bm,
                  float2* out) {
  shapelet_coh_kernel<true>(rows, tab, ch, bm, out);
}

// Array-factor gains of every station toward every (timeslot, source), the
// beam buffer of the predict kernels (kernel_array_beam role,
// predict_model.cu:129; arraybeam, stationbeam.c:49):
//   gain[t,k,n] = below[t,k] ? 0
//               : |(1/nelem[n]) sum_e exp(i kf elem[n,e] . du[t,k])|
// with kf = 2 pi f / c. One thread per (t,k); the block walks AB_NSTA
// consecutive stations, staging each station's elements through LDS in
// tiles of AB_ETILE (any Emax), and every thread sums a station's phasors
// in element order — a fixed order, so results repeat bit for bit. The
// output is strided by N along (t,k); walking AB_NSTA stations per block
// lets each thread write AB_NSTA adjacent floats instead of one, and the
// stores stay 1/nelem of the sincos work. A one-element station has gain 1
// by definition; its rounded cos^2 + sin^2 is not used.
#define AB_ETILE 128
#define AB_NSTA 4

extern "C" __global__ void __launch_bounds__(256)
k_array_beam(const double* __restrict__ elem,   // [N, Emax, 3] ENU, padded
             const int* __restrict__ nelem,     // [N], 1 <= nelem <= Emax
             const double* __restrict__ du,     // [TK, 3]
             const unsigned char* __restrict__ below,  // [TK]
             int N, int Emax, int TK, double kf,
             float* __restrict__ gain) {        // [TK, N]
  __shared__ double ex[AB_ETILE], ey[AB_ETILE], ez[AB_ETILE];
  const int tk = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = tk < TK;
  double dx = 0, dy = 0, dz = 0;
  bool dark = true;
  if (live) {
    dx = kf * du[3 * (size_t)tk];
    dy = kf * du[3 * (size_t)tk + 1];
    dz = kf * du[3 * (size_t)tk + 2];
    dark = below[tk] != 0;
  }
  const int n0 = blockIdx.y * AB_NSTA;
  float g[AB_NSTA];
#pragma unroll
  for (int j = 0; j < AB_NSTA; ++j) {
    g[j] = 0.f;
    const int n = n0 + j;          // block-uniform
    if (n < N) {
      const int ne = nelem[n];
      float re = 0.f, im = 0.f;
      for (int e0 = 0; e0 < ne; e0 += AB_ETILE) {
        const int nt = min(AB_ETILE, ne - e0);
        __syncthreads();
        for (int i = threadIdx.x; i < nt; i += blockDim.x) {
          const double* p = elem + ((size_t)n * Emax + e0 + i) * 3;
          ex[i] = p[0]; ey[i] = p[1]; ez[i] = p[2];
        }
        __syncthreads();
        if (dark) continue;
        for (int i = 0; i < nt; ++i) {
          float s, c;
          sincos_reduced(ex[i] * dx + ey[i] * dy + ez[i] * dz, &s, &c);
          re += c;
          im += s;
        }
      }
      if (!dark)
        g[j] = ne == 1 ? 1.0f : sqrtf(re * re + im * im) / (float)ne;
    }
  }
  if (live) {
#pragma unroll
    for (int j = 0; j < AB_NSTA; ++j)
      if (n0 + j < N) gain[(size_t)tk * N + n0 + j] = g[j];
  }
}

// Station beam gains of every station toward every (timeslot, source) at F
// wavenumbers in one launch, single-stage or two-stage (HBA: an analogue
// tile beam of D dipoles times the digital beam of the tile centroids;
// arraybeam STAT_TILE, stationbeam.c:114; kernel_tile_array_beam role,
// predict_model.cu:236):
//   gain[f,t,k,n] = below[t,k] ? 0
//     : |(1/nelem[n]) sum_e exp(i kf[f] elem[n,e] . du[t,k])|
//       * |(1/D) sum_d exp(i kf[f] tile[n,d] . du_tile[t,k])|
// The second factor is 1 when tile is null (single stage). The structure is
// k_array_beam's: one thread per (t,k), SB_NSTA consecutive stations per
// block, elements staged through LDS in tiles of AB_ETILE (any Emax), the
// dipoles of a station in one pass (D <= SB_DMAX), and every sum taken in
// element order, so results repeat bit for bit. Unlike k_array_beam the
// fp64 dot product e . du is formed once per element WITHOUT kf and then
// scaled by each of the SB_NF wavenumbers the thread carries; blockIdx.z
// walks the frequency axis in passes of SB_NF. A frequency's sum reads only
// its own kf, so its result does not depend on what shares the launch.
//
// SB_NF = 4: per frequency a thread keeps re and im of the running sum (2
// VGPRs) and SB_NSTA finished gains (4); kf is block-uniform and sits in
// SGPRs. So every carried frequency costs 6 VGPRs on top of the ~26 of the
// two directions, the addresses and the fmod/sincos temporaries. Four
// frequencies stay under 64 VGPRs (hipcc reports 50 VGPRs, 92 SGPRs, no
// spills), the most a wave may hold with 8 waves per SIMD resident; the
// loop is fmod + sincos latency chains with no loads to overlap them, so
// those resident waves are what hides it. Eight frequencies would need
// about 24 more VGPRs plus the temporaries of four more chains, by this
// count (an estimate, not compiled) past the 64 that 8 waves per SIMD
// allow, to save the 3 fp64 multiply-adds of the dot product, which at 4
// frequencies are already a small part of the per-element work. F = 256
// is 64 passes along blockIdx.z; a last pass with fewer than SB_NF
// frequencies skips the missing ones. A one-element (one-dipole) stage has
// factor 1 by definition.
#define SB_NF 4
#define SB_NSTA 4
#define SB_DMAX 64

// sum_i exp(i kf[j] (x[i] ux + y[i] uy + z[i] uz)) over nt LDS entries,
// added to re[j], im[j] in entry order, for the nf <= SB_NF frequencies of
// this pass; nf is block-uniform, so the test on it is a scalar branch
__device__ __forceinline__ void sb_accum(const double* x, const double* y,
                                         const double* z, int nt, double ux,
                                         double uy, double uz, int nf,
                                         const double (&kf)[SB_NF],
                                         float (&re)[SB_NF],
                                         float (&im)[SB_NF]) {
  for (int i = 0; i < nt; ++i) {
    const double d = x[i] * ux + y[i] * uy + z[i] * uz;
#pragma unroll
    for (int j = 0; j < SB_NF; ++j) {
      if (j < nf) {
        float s, c;
        sincos_reduced(kf[j] * d, &s, &c);
        re[j] += c;
        im[j] += s;
      }
    }
  }
}

extern "C" __global__ void __launch_bounds__(256)
k_station_beam(const double* __restrict__ elem,   // [N, Emax, 3] ENU, padded
               const int* __restrict__ nelem,     // [N], 1 <= nelem <= Emax
               const double* __restrict__ tile,   // [N, D, 3] or null
               const double* __restrict__ du,     // [TK, 3]
               const double* __restrict__ du_tile,  // [TK, 3], with tile
               const unsigned char* __restrict__ below,  // [TK]
               const double* __restrict__ kfs,    // [F]
               int N, int Emax, int D, int TK, int F,
               float* __restrict__ gain) {        // [F, TK, N]
  __shared__ double ex[AB_ETILE], ey[AB_ETILE], ez[AB_ETILE];
  __shared__ double tx[SB_DMAX], ty[SB_DMAX], tz[SB_DMAX];
  const int tk = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = tk < TK;
  const bool two = tile != nullptr;        // block-uniform
  double ux = 0, uy = 0, uz = 0, vx = 0, vy = 0, vz = 0;
  bool dark = true;
  if (live) {
    ux = du[3 * (size_t)tk];
    uy = du[3 * (size_t)tk + 1];
    uz = du[3 * (size_t)tk + 2];
    if (two) {
      vx = du_tile[3 * (size_t)tk];
      vy = du_tile[3 * (size_t)tk + 1];
      vz = du_tile[3 * (size_t)tk + 2];
    }
    dark = below[tk] != 0;
  }
  const int f0 = blockIdx.z * SB_NF;
  const int nf = min(SB_NF, F - f0);       // block-uniform, >= 1
  double kf[SB_NF];
#pragma unroll
  for (int j = 0; j < SB_NF; ++j) kf[j] = f0 + j < F ? kfs[f0 + j] : 0.0;
  const int n0 = blockIdx.y * SB_NSTA;
  float g[SB_NSTA][SB_NF];
#pragma unroll
  for (int s = 0; s < SB_NSTA; ++s) {
#pragma unroll
    for (int j = 0; j < SB_NF; ++j) g[s][j] = 0.f;
    const int n = n0 + s;            // block-uniform
    if (n < N) {
      const int ne = nelem[n];
      float re[SB_NF], im[SB_NF];
#pragma unroll
      for (int j = 0; j < SB_NF; ++j) re[j] = im[j] = 0.f;
      for (int e0 = 0; e0 < ne; e0 += AB_ETILE) {
        const int nt = min(AB_ETILE, ne - e0);
        __syncthreads();
        for (int i = threadIdx.x; i < nt; i += blockDim.x) {
          const double* p = elem + ((size_t)n * Emax + e0 + i) * 3;
          ex[i] = p[0]; ey[i] = p[1]; ez[i] = p[2];
        }
        __syncthreads();
        if (dark) continue;
        sb_accum(ex, ey, ez, nt, ux, uy, uz, nf, kf, re, im);
      }
      if (!dark) {
#pragma unroll
        for (int j = 0; j < SB_NF; ++j)
          g[s][j] = ne == 1 ? 1.0f
              : sqrtf(re[j] * re[j] + im[j] * im[j]) / (float)ne;
      }
      if (two) {
        __syncthreads();
        for (int i = threadIdx.x; i < D; i += blockDim.x) {
          const double* p = tile + ((size_t)n * D + i) * 3;
          tx[i] = p[0]; ty[i] = p[1]; tz[i] = p[2];
        }
        __syncthreads();
        if (!dark && D > 1) {
#pragma unroll
          for (int j = 0; j < SB_NF; ++j) re[j] = im[j] = 0.f;
          sb_accum(tx, ty, tz, D, vx, vy, vz, nf, kf, re, im);
#pragma unroll
          for (int j = 0; j < SB_NF; ++j)
            g[s][j] *= sqrtf(re[j] * re[j] + im[j] * im[j]) / (float)D;
        }
      }
    }
  }
  if (live) {
#pragma unroll
    for (int j = 0; j < SB_NF; ++j) {
      if (f0 + j >= F) continue;
      float* o = gain + ((size_t)(f0 + j) * TK + tk) * N + n0;
#pragma unroll
      for (int s = 0; s < SB_NSTA; ++s)
        if (n0 + s < N) o[s] = g[s][j];
    }
  }
}
