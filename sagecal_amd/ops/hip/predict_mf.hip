// All-channels coherency predict and fused residual for gfx950 (MI355X):
// the reference's kernel_coherencies and kernel_residuals
// (predict_model.cu:1059, :1242), which carry up to MODEL_MAX_F channels
// per thread, with the station beam in compile-time variants like the
// dobeam branches of those two kernels. No shapelet sources here (shapelet
// fluxes arrive zeroed, as for k_predict_coh); packs that have them stay
// with the per-channel kernels of predict.hip.
//
// One body, predict_mf_body, templated on a sink, on the channels a thread
// carries per pass and on the beam variant. One thread per row
// r = t*Nbase + b; the sources of a cluster are staged through LDS in tiles
// of SRC_TILE together with their fluxes at the MF_NF channels of the pass;
// a thread carries the Stokes sums of MF_NF channels. Per source and row,
// once: the fp64 phase term G, the frequency smearing (a function of
// G*fdelta2), the projected (u', v') per Hz and the gaussian's sincos(eP).
// Per channel: the fp64 reduction of G*freq with the fast sincos and the
// time smearing (sincos_reduced and time_smear of predict.hip, the
// expressions of k_predict_coh, so a point source gives the same bits as
// there), and the envelope at (u', v') * freq. The envelope differs from
// k_predict_coh's in rounding only: that kernel rounds u*freq to float and
// then rotates, this one rotates the float u and then scales by the float
// freq.
//
// A channel's sums read its own frequency and its own fluxes and nothing
// of the other channels, and sources are added in source order, so its
// result does not depend on what shares its pass or launch.
//
// Sinks (pass(): after each pass of a cluster, sums of nf channels from f0;
// cluster(): after a cluster's last pass; finish(): after the last cluster;
// all three on live rows only):
//   k_predict_coh_mf    stores out[f, ci, r, :]; passes along blockIdx.z.
//   k_predict_coh_mean  adds the channels' coherencies in channel order,
//                       passes inside the thread, stores the sum / F: a
//                       fixed order, so results repeat bit for bit.
//   k_residual_mf       adds J_p C J_q^H of every subtracted cluster to a
//                       running model per channel (k_apply_jones's order:
//                       C J_q^H, then J_p times it) and stores x - model;
//                       C never leaves the registers. Passes along
//                       blockIdx.z. Clusters with skip[ci] != 0 (solved but
//                       not subtracted, residual.c:74) are left out before
//                       their sources are staged, a block-uniform branch.
//
// Beam variants of all three sinks (template parameter BM, chosen at launch
// from BeamChannels; the plain entries carry no beam code and no branch for
// it, and compile to the instructions they had before, differently
// scheduled: their results are bit for bit what they were):
//   _bm  scalar station gains (-B 1/4): every source is scaled by
//        beam[f, t, k, p] * beam[f, t, k, q]; Stokes sums as without beam.
//   _ej  E-Jones sandwich (-B 2/3/5/6), gains optional: every source adds
//        g_p g_q E_p C E_q^H with E_s = ejones[f, t, k, s or 0, :, :], so
//        the sums are the four coherency entries.
// Both go through beam_row, add_source<EJ> and put_coherency<EJ> of
// predict.hip, the per-source arithmetic of k_predict_coh[_ej]. Channel j of
// a pass reads row f0 + j of both buffers, a block-uniform offset. A row
// whose pair has a negative entry (k_residual_mf keeps x there) would index
// the buffers with that station: with a beam such a row is not `lit`, skips
// the source loop like a row past R, and forms no beam address; its sums
// stay zero and the sink still stores x.
//
// MF_NF = 2. Per carried channel a thread holds the 8 floats of the
// cluster's Stokes sums, and k_residual_mf the 8 of the running model as
// well; frequencies are block-uniform and sit in SGPRs. hipcc -O3 for
// gfx950, -Rpass-analysis=kernel-resource-usage, VGPRs / waves per SIMD
// (every entry: 106 SGPRs, no scratch; k_predict_coh itself: 97 / 5):
//              k_predict_coh_mf   k_predict_coh_mean   k_residual_mf
//   MF_NF = 2       127 / 4            136 / 3            146 / 3
//   MF_NF = 4       165 / 3            175 / 2            199 / 2
//   MF_NF = 8       254 / 2            254 / 2            256 / 1
// At 8 the residual kernel fills all 256 VGPRs and parks 48 more values in
// AGPRs: no scratch, but spills in all but name, and one wave per SIMD.
// Accepted: 2, at 3 to 4 waves per SIMD. The source loop is fmod + sincos +
// erff latency chains with no loads to overlap, hidden by the independent
// chains a SIMD holds, waves times carried channels: 5 for k_predict_coh,
// 6 to 8 here at 2, 8 to 12 at 4, 8 to 16 at 8. By that count 4 should do
// no worse than 2, so all three were timed on an MI355X
// (tools/bench_residual_predict.py: 1,935,360 rows, 8 channels, 50 point
// sources; calculate_residuals_multifreq / precalc_coherencies, ms):
// 2.83 / 2.40 at 2, 3.16 / 2.70 at 4, 5.42 / 2.50 at 8. Resident waves
// count for more than channels per wave; what 4 saves in shared per-source
// work (G, the sinc and its division, the LDS reads) does not make up for
// the wave it costs.
//
// The beam variants, same compiler and flags (106 SGPRs, no scratch, no
// AGPRs throughout). _bm at MF_NF = 2 adds the two gain loads per source
// and channel:
//              k_predict_coh_mf_bm  k_predict_coh_mean_bm  k_residual_mf_bm
//   MF_NF = 2       128 / 4             142 / 3               152 / 3
// _ej holds per carried channel the 8 floats of the coherency sums (and the
// 8 of the running model) plus, per source, two 2x2 patterns and the two
// products of the sandwich, so it has a constant of its own, MF_NF_EJ:
//              k_predict_coh_mf_ej  k_predict_coh_mean_ej  k_residual_mf_ej
//   MF_NF_EJ = 1    115 / 4             125 / 4               125 / 4
//   MF_NF_EJ = 2    143 / 3             167 / 3               169 / 2
//   MF_NF_EJ = 4    179 / 2             194 / 2               210 / 2
// By the table 1 keeps 4 waves everywhere and 2 drops the residual kernel
// to 2 waves by one register. Timed on an MI355X like the above
// (tools/bench_residual_predict.py --beam MODE, NE = 1;
// calculate_residuals_multifreq / channel-mean predict, ms; the per-channel
// loop takes 13.9 / 8.1 with gains and patterns, 12.9 / 7.2 with patterns):
//                     gains and patterns     patterns alone
//   MF_NF_EJ = 1         6.07 / 5.98           5.38 / 5.28
//   MF_NF_EJ = 2         7.51 / 5.65           5.84 / 4.80
//   MF_NF_EJ = 4         7.10 / 6.87           5.30 / 5.27
// Accepted: 1. The residual runs for every -B mode and gains 8 to 19 % over
// 2; the mean runs for -B 5/6 only and loses 6 to 10 %. _bm at MF_NF = 2:
// 4.06 / 3.78 against 11.6 / 5.97 for the loop.
#define MF_NF PREDICT_MF_NF
#define MF_NF_EJ PREDICT_MF_NF_EJ

// Compile-time beam variant of the body, as template <bool EJ> in
// predict.hip: the plain entries carry no beam code and no branch for it.
#define MF_PLAIN 0   // no beam
#define MF_GAIN 1    // scalar station gains (-B 1/4)
#define MF_EJ 2      // E-Jones sandwich, gains optional (-B 2/3/5/6)

template <int NF>
struct SrcTileMF {
  double ll[SRC_TILE], mm[SRC_TILE], nn1[SRC_TILE];
  float flux[NF][4][SRC_TILE];  // per channel of the pass: I,Q,U,V
  float eX[SRC_TILE], eY[SRC_TILE], eP[SRC_TILE];
  float cxi[SRC_TILE], sxi[SRC_TILE], cphi[SRC_TILE], sphi[SRC_TILE];
  float r1[SRC_TILE];
  int   stype[SRC_TILE];
};

// Passes pass0 <= pass < pass1 of NF channels each, for every cluster.
// With BM != MF_PLAIN, channel f reads beam[f, t, k, s] and
// ejones[f, t, k, e, :, :] (rows bstride floats and estride float2 apart),
// t = r / Nbase and s, e from pairs; R == T * Nbase.
template <int NF, int BM, typename Sink>
__device__ __forceinline__ void predict_mf_body(
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
    int M, const double* __restrict__ freqs, int F, double fdelta2,
    double tdelta, size_t fstride, const int* __restrict__ skip,
    const float* __restrict__ beam, const float2* __restrict__ ejones,
    const int* __restrict__ pairs, int Nbase, int Ktot, int Nsta, int NE,
    size_t bstride, size_t estride, int pass0, int pass1, Sink& sink) {
  constexpr bool EJ = BM == MF_EJ;
  __shared__ SrcTileMF<NF> tile;
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = r < R;
  double ur = 0, vr = 0, wr = 0, bl = 0;
  if (live) {
    ur = u[r]; vr = v[r]; wr = w[r];
    bl = sqrt(ur * ur + vr * vr + wr * wr);
  }
  const float uh = (float)ur, vh = (float)vr, wh = (float)wr;   // per Hz
  const BeamRow br = BM == MF_PLAIN ? BeamRow{0, 0, 0, 0, 0}
                                    : beam_row(live, r, pairs, Nbase, Ktot,
                                               NE);
  // `lit` rows walk the sources. With a beam, a row whose pair has a
  // negative entry (k_residual_mf keeps x there) is not lit: its stations
  // index no beam buffer, and its sums stay zero.
  const bool lit = BM == MF_PLAIN ? live
                                  : live && br.sta1 >= 0 && br.sta2 >= 0;

  for (int ci = 0; ci < M; ++ci) {
    if (skip != nullptr && skip[ci] != 0) continue;    // block-uniform
    const int s0 = cluster_off[ci], s1 = cluster_off[ci + 1];
    for (int pass = pass0; pass < pass1; ++pass) {
      const int f0 = pass * NF;
      const int nf = min(NF, F - f0);                  // block-uniform, >= 1
      double fq[NF];
      float ff[NF], tsm_c[NF];
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        fq[j] = j < nf ? freqs[f0 + j] : 0.0;
        ff[j] = (float)fq[j];
        tsm_c[j] = 7.2921150e-5f * (float)tdelta * (float)(bl * fq[j]);
      }
      // sums of add_source per channel: Stokes IIl/QQl/UUl/VVl, or with EJ
      // the four coherency entries
      cf acc[NF][4];
#pragma unroll
      for (int j = 0; j < NF; ++j)
        for (int i = 0; i < 4; ++i) acc[j][i] = {0.f, 0.f};
      for (int base = s0; base < s1; base += SRC_TILE) {
        const int nt = min(SRC_TILE, s1 - base);
        __syncthreads();
        for (int k = threadIdx.x; k < nt; k += blockDim.x) {
          const int g = base + k;
          tile.ll[k] = ll[g];   tile.mm[k] = mm[g];   tile.nn1[k] = nn1[g];
#pragma unroll
          for (int j = 0; j < NF; ++j) {
            if (j < nf) {
              const size_t fg = (size_t)(f0 + j) * fstride + g;
              tile.flux[j][0][k] = sI[fg];   tile.flux[j][1][k] = sQ[fg];
              tile.flux[j][2][k] = sU[fg];   tile.flux[j][3][k] = sV[fg];
            }
          }
          tile.eX[k] = eX[g];   tile.eY[k] = eY[g];   tile.eP[k] = eP[g];
          tile.cxi[k] = cxi[g]; tile.sxi[k] = sxi[g];
          tile.cphi[k] = cphi[g]; tile.sphi[k] = sphi[g];
          tile.r1[k] = r1t[g];  tile.stype[k] = stype[g];
        }
        __syncthreads();
        if (!lit) continue;
        for (int k = 0; k < nt; ++k) {
          const double G = phase_term(ur, vr, wr, tile.ll[k], tile.mm[k],
                                      tile.nn1[k]);
          const float sm = freq_smear(G, fdelta2);
          const float r1 = tile.r1[k];
          // extended source: projection rotation of the row's (u,v,w) per
          // Hz (predict.c:36-44; the host bakes use_projection into
          // cxi/sxi/cphi/sphi), and the gaussian's position angle
          const int st = tile.stype[k];
          float up = 0.f, vp = 0.f, cpp = 1.f, spp = 0.f;
          if (st != 0) {
            const float c_xi = tile.cxi[k], s_xi = tile.sxi[k];
            const float c_ph = tile.cphi[k], s_ph = tile.sphi[k];
            up = uh * c_xi - vh * c_ph * s_xi + wh * s_ph * s_xi;
            vp = uh * s_xi + vh * c_ph * c_xi - wh * s_ph * c_xi;
            if (st == 1) __sincosf(tile.eP[k], &spp, &cpp);
          }
#pragma unroll
          for (int j = 0; j < NF; ++j) {
            if (j < nf) {                              // block-uniform
              float sp, cp;
              sincos_reduced(fma(G, fq[j], 0.0), &sp, &cp);
              const float smj = time_smear(sm, tsm_c[j], r1);
              cf phc = {cp * smj, sp * smj};
              if (st != 0) {
                // envelope at the wavelength-scaled (u', v')
                const float upf = up * ff[j], vpf = vp * ff[j];
                if (st == 1) {  // gaussian
                  const float ut = tile.eX[k] * (cpp * upf - spp * vpf);
                  const float vt = tile.eY[k] * (spp * upf + cpp * vpf);
                  phc = cscale(phc, __expf(-19.739208802178716f *
                                           (ut * ut + vt * vt)));
                } else if (st == 2) {  // disk: j1
                  const float b = sqrtf(upf * upf + vpf * vpf) * tile.eX[k] *
                                  6.2831853071795865f;
                  phc = cscale(phc, j1f(b));
                } else if (st == 3) {  // ring: j0
                  const float b = sqrtf(upf * upf + vpf * vpf) * tile.eX[k] *
                                  6.2831853071795865f;
                  phc = cscale(phc, j0f(b));
                }
                // st==4 (shapelet): fluxes are zero here
              }
              if constexpr (BM == MF_PLAIN) {
                add_source<false>(phc,
                                  [&](int i) { return tile.flux[j][i][k]; },
                                  base + k, br, nullptr, 0, nullptr, 0,
                                  acc[j]);
              } else {
                // row f0 + j of the beam buffers (block-uniform offsets)
                const size_t fj = (size_t)(f0 + j);
                add_source<EJ>(
                    phc, [&](int i) { return tile.flux[j][i][k]; }, base + k,
                    br, beam != nullptr ? beam + fj * bstride : nullptr, Nsta,
                    EJ ? ejones + fj * estride : nullptr, NE, acc[j]);
              }
            }
          }
        }
      }
      if (live) sink.pass(ci, f0, nf, acc);
    }
    if (live) sink.cluster(ci);
  }
  if (live) sink.finish();
}

// The one place that unpacks the argument structs of this kernel family.
template <int NF, int BM, typename Sink>
__device__ __forceinline__ void predict_mf_kernel(
    const RowsUVW& rows, const SourceArrays& s, const Channels& ch,
    const BeamChannels& bm, const int* __restrict__ skip, int pass0,
    int pass1, Sink& sink) {
  predict_mf_body<NF, BM>(
      rows.u, rows.v, rows.w, rows.R, s.ll, s.mm, s.nn1, s.sI, s.sQ, s.sU,
      s.sV, s.eX, s.eY, s.eP, s.cxi, s.sxi, s.cphi, s.sphi, s.r1, s.stype,
      s.cluster_off, s.M, ch.freqs, ch.F, ch.fdelta2, ch.tdelta,
      (size_t)ch.flux_stride, skip, BM != MF_PLAIN ? bm.beam : nullptr,
      BM == MF_EJ ? bm.ejones : nullptr, bm.pairs, bm.Nbase, bm.Ktot,
      bm.Nsta, BM == MF_EJ ? bm.NE : 0,
      (size_t)bm.T * bm.Ktot * bm.Nsta, (size_t)bm.T * bm.Ktot * bm.NE * 4,
      pass0, pass1, sink);
}

// out[f, ci, r, :] of every channel of the pass
template <int NF, bool EJ>
struct StoreSink {
  float2* __restrict__ out;   // [F, M, R, 4]
  int r, R, M;
  __device__ __forceinline__ void pass(int ci, int f0, int nf,
                                       const cf (&acc)[NF][4]) {
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      if (j < nf) {
        float2* o = out + (((size_t)(f0 + j) * M + ci) * R + r) * 4;
        put_coherency<EJ>(acc[j], [&](int i, cf c) { o[i] = c; });
      }
    }
  }
  __device__ __forceinline__ void cluster(int) {}
  __device__ __forceinline__ void finish() {}
};

// out[ci, r, :] = (sum over channels, in channel order) / F
template <int NF, bool EJ>
struct MeanSink {
  float2* __restrict__ out;   // [M, R, 4]
  int r, R, F;
  cf m[4];
  __device__ __forceinline__ void pass(int, int, int nf,
                                       const cf (&acc)[NF][4]) {
#pragma unroll
    for (int j = 0; j < NF; ++j)
      if (j < nf)
        put_coherency<EJ>(acc[j],
                          [&](int i, cf c) { m[i] = cadd(m[i], c); });
  }
  __device__ __forceinline__ void cluster(int ci) {
    float2* o = out + ((size_t)ci * R + r) * 4;
    const float nch = (float)F;
    for (int i = 0; i < 4; ++i) {
      o[i] = {m[i].x / nch, m[i].y / nch};
      m[i] = {0.f, 0.f};
    }
  }
  __device__ __forceinline__ void finish() {}
};

// out[f, r, :] = x[f, r, :] - sum over clusters of J_p C J_q^H
template <int NF, bool EJ>
struct ResidualSink {
  float2* __restrict__ out;        // [F, R, 4]
  const float2* __restrict__ x;    // [F, R, 4]
  const float2* __restrict__ J;    // [Mt, N, 4]
  const int* __restrict__ chunk;   // chunk_tab + t, strided by T along ci
  int r, R, T, N;
  int p, q;                        // stations of the row; p < 0: keep x
  int f0, nf;
  cf model[NF][4];
  __device__ __forceinline__ void pass(int ci, int f0_, int nf_,
                                       const cf (&acc)[NF][4]) {
    f0 = f0_;
    nf = nf_;
    if (p < 0) return;
    const int c = chunk[(size_t)ci * T];
    cf J1[4], J2[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      J1[i] = J[((size_t)c * N + p) * 4 + i];
      J2[i] = J[((size_t)c * N + q) * 4 + i];
    }
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      if (j < nf) {
        cf C[4], G1[4], V[4];
        put_coherency<EJ>(acc[j], [&](int i, cf c_) { C[i] = c_; });
        m2mulh(C, J2, G1);
        m2mul(J1, G1, V);
#pragma unroll
        for (int i = 0; i < 4; ++i) model[j][i] = cadd(model[j][i], V[i]);
      }
    }
  }
  __device__ __forceinline__ void cluster(int) {}
  __device__ __forceinline__ void finish() {
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      if (j < nf) {
        const size_t o = ((size_t)(f0 + j) * R + r) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          out[o + i] = p < 0 ? x[o + i] : csub(x[o + i], model[j][i]);
      }
    }
  }
};

// The three entries, each for every beam variant. Passes along blockIdx.z,
// except the mean, whose threads walk the passes themselves.
template <int NF, int BM>
__device__ __forceinline__ void coh_mf_entry(
    const RowsUVW& rows, const SourceArrays& src, const Channels& ch,
    const BeamChannels& bm, float2* __restrict__ out) {
  StoreSink<NF, BM == MF_EJ> sink = {
      out, (int)(blockIdx.x * blockDim.x + threadIdx.x), rows.R, src.M};
  predict_mf_kernel<NF, BM>(rows, src, ch, bm, nullptr, blockIdx.z,
                            blockIdx.z + 1, sink);
}

template <int NF, int BM>
__device__ __forceinline__ void coh_mean_entry(
    const RowsUVW& rows, const SourceArrays& src, const Channels& ch,
    const BeamChannels& bm, float2* __restrict__ out) {
  MeanSink<NF, BM == MF_EJ> sink = {
      out, (int)(blockIdx.x * blockDim.x + threadIdx.x), rows.R, ch.F,
      {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}}};
  predict_mf_kernel<NF, BM>(rows, src, ch, bm, nullptr, 0,
                            (ch.F + NF - 1) / NF, sink);
}

// rows.R == res.T * res.Nbase (the launcher checks it)
template <int NF, int BM>
__device__ __forceinline__ void residual_mf_entry(
    const RowsUVW& rows, const SourceArrays& src, const Channels& ch,
    const BeamChannels& bm, const ResidualArgs& res,
    float2* __restrict__ out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  ResidualSink<NF, BM == MF_EJ> sink = {};
  sink.out = out;  sink.x = res.x;  sink.J = res.J;
  sink.r = r;  sink.R = rows.R;  sink.T = res.T;  sink.N = res.N;
  sink.p = -1;
  // a pass that finds every cluster skipped still stores x
  sink.f0 = blockIdx.z * NF;
  sink.nf = min(NF, ch.F - sink.f0);
  if (r < rows.R) {
    const int t = r / res.Nbase, b = r - t * res.Nbase;
    sink.p = res.pairs[2 * b];
    sink.q = res.pairs[2 * b + 1];
    if (sink.q < 0) sink.p = -1;
    sink.chunk = res.chunk_tab + t;
  }
  predict_mf_kernel<NF, BM>(rows, src, ch, bm, res.skip, blockIdx.z,
                            blockIdx.z + 1, sink);
}

extern "C" __global__ void __launch_bounds__(128)
k_predict_coh_mf(RowsUVW rows, SourceArrays src, Channels ch,
                 float2* __restrict__ out) {
  coh_mf_entry<MF_NF, MF_PLAIN>(rows, src, ch, BeamChannels{}, out);
}

extern "C" __global__ void __launch_bounds__(128)
k_predict_coh_mean(RowsUVW rows, SourceArrays src, Channels ch,
                   float2* __restrict__ out) {
  coh_mean_entry<MF_NF, MF_PLAIN>(rows, src, ch, BeamChannels{}, out);
}

extern "C" __global__ void __launch_bounds__(128)
k_residual_mf(RowsUVW rows, SourceArrays src, Channels ch, ResidualArgs res,
              float2* __restrict__ out) {
  residual_mf_entry<MF_NF, MF_PLAIN>(rows, src, ch, BeamChannels{}, res, out);
}

// Scalar-gain variants: bm.beam, bm.pairs required.
extern "C" __global__ void __launch_bounds__(128)
k_predict_coh_mf_bm(RowsUVW rows, SourceArrays src, Channels ch,
                    BeamChannels bm, float2* __restrict__ out) {
  coh_mf_entry<MF_NF, MF_GAIN>(rows, src, ch, bm, out);
}

extern "C" __global__ void __launch_bounds__(128)
k_predict_coh_mean_bm(RowsUVW rows, SourceArrays src, Channels ch,
                      BeamChannels bm, float2* __restrict__ out) {
  coh_mean_entry<MF_NF, MF_GAIN>(rows, src, ch, bm, out);
}

extern "C" __global__ void __launch_bounds__(128)
k_residual_mf_bm(RowsUVW rows, SourceArrays src, Channels ch,
                 BeamChannels bm, ResidualArgs res,
                 float2* __restrict__ out) {
  residual_mf_entry<MF_NF, MF_GAIN>(rows, src, ch, bm, res, out);
}

// E-Jones variants: bm.ejones, bm.pairs required; bm.beam may be null.
extern "C" __global__ void __launch_bounds__(128)
k_predict_coh_mf_ej(RowsUVW rows, SourceArrays src, Channels ch,
                    BeamChannels bm, float2* __restrict__ out) {
  coh_mf_entry<MF_NF_EJ, MF_EJ>(rows, src, ch, bm, out);
}

extern "C" __global__ void __launch_bounds__(128)
k_predict_coh_mean_ej(RowsUVW rows, SourceArrays src, Channels ch,
                      BeamChannels bm, float2* __restrict__ out) {
  coh_mean_entry<MF_NF_EJ, MF_EJ>(rows, src, ch, bm, out);
}

extern "C" __global__ void __launch_bounds__(128)
k_residual_mf_ej(RowsUVW rows, SourceArrays src, Channels ch,
                 BeamChannels bm, ResidualArgs res,
                 float2* __restrict__ out) {
  residual_mf_entry<MF_NF_EJ, MF_EJ>(rows, src, ch, bm, res, out);
}
