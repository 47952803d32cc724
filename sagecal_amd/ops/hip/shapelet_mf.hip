// All-channels shapelet predict and residual for gfx950 (MI355X): the
// shapelet branch of the reference's kernel_coherencies and
// kernel_residuals (predict_model.cu:1059, :1242), which carry shapelet
// sources through their MODEL_MAX_F channel loop like any other type. Here
// they are k_shapelet_coh (predict.hip) for every channel of a tile in one
// launch, added into what the kernels of predict_mf.hip have written: each
// entry below is launched after its predict_mf.hip counterpart on the same
// stream, into the same buffer, with the same beam, pairs, skip and chunk
// table. Every (cluster, row, channel) belongs to one thread: no atomics.
//
// One body, shapelet_mf_body, templated like predict_mf_body on the
// channels a thread carries per pass, the beam variant and a sink. One
// thread per row r = t*Nbase + b in blocks of 128. The loops over clusters,
// passes and table entries are block-uniform and the table is reached
// through the __restrict__ parameters of the body (the forwarding rule of
// predict.hip), so every table, coefficient, recurrence-constant, frequency
// and flux read is a scalar-cache load; nothing goes through LDS and there
// is no barrier. Clusters are walked through the [M + 1] prefix of table
// entries per cluster (ShapeletTable.entry_off), so the loop nest is
// cluster, pass of NF channels, entry; a cluster without entries is left
// before anything is computed and nothing is stored for it.
//
// Per entry and row, once: the fp64 phase term, the frequency smearing and
// the entry's constants. Per carried channel: the fp64 phase reduction with
// the fast sincos, the time smearing, the wavelength-scaled (float)(u*freq)
// and the rotation, psign, a/b and position-angle arithmetic, all in the
// expressions and order of shapelet_coh_body, so a channel differs from
// k_shapelet_coh at that frequency in instruction scheduling at most. The
// Hermite double loop (n2 outer, n1 inner, no per-thread arrays, no cap on
// n0) runs for the NF channels together: each coefficient and each pair of
// recurrence constants is read once and feeds NF independent recurrence
// chains. In k_shapelet_coh a step of the inner loop is a serial dependency
// chain of two multiply-adds; interleaving the channels' chains fills its
// latency, which is what this kernel gains beyond the shared per-row work.
// A pass with fewer than NF channels runs the spare chains on zeros and
// adds nothing for them. A channel's sums read its own frequency, fluxes
// and beam rows only and entries are added in table order, so its result
// does not depend on what shares its pass or launch.
//
// Sinks, all additive:
//   k_shapelet_coh_mf    out[f, ci, r, :] += C; passes along blockIdx.z.
//   k_shapelet_coh_mean  sums the channels' coherencies in channel order,
//                        passes inside the thread, then
//                        out[ci, r, :] += sum / F: results repeat bit for
//                        bit.
//   k_shapelet_residual_mf  per cluster with entries and skip[ci] == 0 adds
//                        J_p C J_q^H to a running model per channel
//                        (ResidualSink's order: m2mulh, then m2mul), then
//                        out[f, r, :] -= model. Passes along blockIdx.z. A
//                        row with a negative pair entry leaves at once and
//                        keeps what the main kernel stored (x); if every
//                        cluster with entries is skipped nothing is touched.
// Beam variants as in predict_mf.hip (BM; beam_row, add_source<EJ>,
// put_coherency<EJ> of predict.hip; the beam is indexed by the table's
// src[s]): plain, _bm (beam[f,t,k,p] * beam[f,t,k,q]) and _ej
// (g_p g_q E_p C E_q^H). A row whose pair has a negative entry forms no
// beam address.
//
// Per carried channel a thread holds pu, pu1, pv, pv1, se, so, re, im, xu,
// xv, pu0 and the 8 floats of the sums, the residual kernel the 8 of the
// running model too. hipcc -O3 for gfx950,
// -Rpass-analysis=kernel-resource-usage, VGPRs / waves per SIMD as the
// compiler reports them (every entry: 106 SGPRs, no scratch, no AGPRs;
// k_shapelet_coh itself: 50 / 7, k_shapelet_coh_ej 69 / 7):
//              k_shapelet_coh_mf  k_shapelet_coh_mean  k_shapelet_residual_mf
//   NF = 1          44 / 7             62 / 7               66 / 7
//   NF = 2          73 / 6             80 / 6              125 / 4
//   NF = 4         128 / 4            133 / 3              178 / 2
//              ..._coh_mf_bm      ..._coh_mean_bm      ..._residual_mf_bm
//   NF = 1          50 / 7             68 / 7               72 / 7
//   NF = 2          77 / 6             86 / 5              131 / 3
//   NF = 4         131 / 3            139 / 3              185 / 2
//              ..._coh_mf_ej      ..._coh_mean_ej      ..._residual_mf_ej
//   NF_EJ = 1       75 / 6             83 / 5               88 / 5
//   NF_EJ = 2       95 / 5            104 / 4              149 / 3
//   NF_EJ = 4      135 / 3            144 / 3              189 / 2
// The NF = 2 entries without beam have 51 to 58 scalar load instructions
// (s_load) and 5 to 13 per-lane ones (the row's u, v, w, out, and J in the
// residual).
//
// Timed on an MI355X (tools/bench_residual_predict.py --shapelets 32,8:
// 1,935,360 rows, 8 channels, 50 sources of which 32 are shapelets with
// n0 = 8; calculate_residuals_multifreq / channel-mean predict, ms, median
// of 10, main and shapelet launch together; profiles/shapelet_multifreq.json
// has the 2-source n0 = 3 sky and the spreads):
//                 no beam          gains (--beam 1)   patterns (--beam 3)
//   NF = 1      16.75 / 16.91      18.06 / 18.45       20.00 / 20.63
//   NF = 2      12.49 / 11.25      15.89 / 13.38       17.48 / 16.04
//   NF = 4      13.93 / 11.22      16.22 / 13.12       17.64 / 15.12
//   loop        25.6  / 19.7       26.9  / 20.9        28.3  / 22.2
// (the patterns column sweeps NF_EJ). Accepted: SHAPELET_MF_NF = 2 and
// SHAPELET_MF_NF_EJ = 2, the fastest on the residual. The second chain is
// what pays: 1 -> 2 saves 2 to 4 ms on the residual and 5 ms on the mean,
// at 6 waves instead of 7. At 4 the store and mean kernels hold their
// speed at 3 to 4 waves (the mean with patterns gains 0.9 ms), but the
// residual kernels drop to 2 waves and lose 0.2 to 1.4 ms; with patterns
// the 0.16 ms between 2 and 4 is inside the run-to-run spread (0.2 to
// 0.35 ms), so 2 is kept there for its registers, not for that figure. On
// the 2-source sky the three values are within 0.15 ms of each other.
// "loop" is the per-channel loop (k_predict_coh, k_shapelet_coh,
// k_apply_jones per channel), whose spread over 10 calls is 0.1 to 0.2 ms.
#define SH_NF SHAPELET_MF_NF
#define SH_NF_EJ SHAPELET_MF_NF_EJ

// The entries are compiled without the packed fp32 instructions
// (v_pk_add/mul/fma_f32): left alone the compiler pairs the chains of two
// channels into them. The chains stay NF separate v_fma_f32 streams, the
// same instruction sequence for a channel in every slot of a pass, and the
// register tables and timings above are of that code.
#define SH_NO_PK __attribute__((target("no-packed-fp32-ops")))

// Passes pass0 <= pass < pass1 of NF channels each, for every cluster with
// table entries. Beam arguments as for predict_mf_body; flux [F, 4, S] with
// rows fstride floats apart.
template <int NF, int BM, typename Sink>
__device__ __forceinline__ void shapelet_mf_body(
    const double* __restrict__ u, const double* __restrict__ v,
    const double* __restrict__ w, int R,
    const int* __restrict__ src, const int* __restrict__ n0t,
    const float* __restrict__ betat, const int* __restrict__ off,
    const float* __restrict__ coef, const float* __restrict__ cxi,
    const float* __restrict__ sxi, const float* __restrict__ cphi,
    const float* __restrict__ sphi, const float* __restrict__ psign,
    const float* __restrict__ at, const float* __restrict__ bt,
    const float* __restrict__ ceP, const float* __restrict__ seP,
    const double* __restrict__ ll, const double* __restrict__ mm,
    const double* __restrict__ nn1, const float* __restrict__ rec, int S,
    int nmax, const float* __restrict__ flux, const float* __restrict__ r1t,
    const int* __restrict__ entry_off, int M,
    const double* __restrict__ freqs, int F, double fdelta2, double tdelta,
    size_t fstride, const int* __restrict__ skip,
    const float* __restrict__ beam, const float2* __restrict__ ejones,
    const int* __restrict__ pairs, int Nbase, int Ktot, int Nsta, int NE,
    size_t bstride, size_t estride, int pass0, int pass1, Sink& sink) {
  constexpr bool EJ = BM == MF_EJ;
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const BeamRow br = BM == MF_PLAIN ? BeamRow{0, 0, 0, 0, 0}
                                    : beam_row(true, r, pairs, Nbase, Ktot,
                                               NE);
  // a row whose pair has a negative entry indexes no beam buffer; every
  // sink is additive, so it has nothing to do
  if (BM != MF_PLAIN && (br.sta1 < 0 || br.sta2 < 0)) return;
  const double ur = u[r], vr = v[r], wr = w[r];
  const double bl = sqrt(ur * ur + vr * vr + wr * wr);
  const float* rec0 = rec;          // sqrt(2/n)
  const float* rec1 = rec + nmax;   // sqrt((n-1)/n)

  for (int ci = 0; ci < M; ++ci) {
    const int e0 = entry_off[ci], e1 = entry_off[ci + 1];
    if (e0 == e1) continue;                            // block-uniform
    if (skip != nullptr && skip[ci] != 0) continue;    // block-uniform
    for (int pass = pass0; pass < pass1; ++pass) {
      const int f0 = pass * NF;
      const int nf = min(NF, F - f0);                  // block-uniform, >= 1
      double fq[NF];
      float uf[NF], vf[NF], wf[NF], tsm_c[NF];
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        fq[j] = j < nf ? freqs[f0 + j] : 0.0;
        const float blf = (float)(bl * fq[j]);
        uf[j] = (float)(ur * fq[j]);
        vf[j] = (float)(vr * fq[j]);
        wf[j] = (float)(wr * fq[j]);
        tsm_c[j] = 7.2921150e-5f * (float)tdelta * blf;
      }
      // sums of add_source per channel, as in predict_mf_body
      cf acc[NF][4];
#pragma unroll
      for (int j = 0; j < NF; ++j)
        for (int i = 0; i < 4; ++i) acc[j][i] = {0.f, 0.f};
      for (int s = e0; s < e1; ++s) {
        const double G = phase_term(ur, vr, wr, ll[s], mm[s], nn1[s]);
        const float sm = freq_smear(G, fdelta2);
        const float r1 = r1t[s];
        const float c_xi = cxi[s], s_xi = sxi[s];
        const float c_ph = cphi[s], s_ph = sphi[s];
        const float beta = betat[s];
        const int n0 = n0t[s];
        const float* cf_s = coef + off[s];
        cf phc[NF];
        float xu[NF], xv[NF], pu0[NF], pv[NF], pv1[NF], re[NF], im[NF];
#pragma unroll
        for (int j = 0; j < NF; ++j) {
          phc[j] = {0.f, 0.f};
          xu[j] = xv[j] = pu0[j] = pv[j] = pv1[j] = re[j] = im[j] = 0.f;
          if (j < nf) {                                // block-uniform
            float sp, cp;
            sincos_reduced(fma(G, fq[j], 0.0), &sp, &cp);
            const float smj = time_smear(sm, tsm_c[j], r1);
            phc[j] = {cp * smj, sp * smj};
            const float up = psign[s] *
                (uf[j] * c_xi - vf[j] * c_ph * s_xi + wf[j] * s_ph * s_xi);
            const float vp = psign[s] *
                (uf[j] * s_xi + vf[j] * c_ph * c_xi - wf[j] * s_ph * c_xi);
            const float ut = at[s] * (ceP[s] * up - seP[s] * vp);
            const float vt = bt[s] * (seP[s] * up + ceP[s] * vp);
            xu[j] = -ut * beta;
            xv[j] = vt * beta;
            pu0[j] = 0.70710678118654752f * expf(-0.5f * xu[j] * xu[j]);
            pv[j] = 0.70710678118654752f * expf(-0.5f * xv[j] * xv[j]);
          }
        }
        for (int n2 = 0; n2 < n0; ++n2) {
          if (n2 > 0) {
            const float a2 = rec0[n2], b2 = rec1[n2];
#pragma unroll
            for (int j = 0; j < NF; ++j) {
              const float t = xv[j] * a2 * pv[j] - b2 * pv1[j];
              pv1[j] = pv[j];
              pv[j] = t;
            }
          }
          // row sums over even and odd n1, NF chains side by side
          float se[NF], so[NF], pu1[NF], pu[NF];
#pragma unroll
          for (int j = 0; j < NF; ++j) {
            se[j] = so[j] = pu1[j] = 0.f;
            pu[j] = pu0[j];
          }
          const float* c = cf_s + n2 * n0;
          for (int n1 = 0; n1 < n0; ++n1) {
            if (n1 > 0) {
              const float a1 = rec0[n1], b1 = rec1[n1];
#pragma unroll
              for (int j = 0; j < NF; ++j) {
                const float t = xu[j] * a1 * pu[j] - b1 * pu1[j];
                pu1[j] = pu[j];
                pu[j] = t;
              }
            }
            const float cn = c[n1];
#pragma unroll
            for (int j = 0; j < NF; ++j) {
              if (n1 & 1) so[j] += cn * pu[j];
              else        se[j] += cn * pu[j];
            }
          }
#pragma unroll
          for (int j = 0; j < NF; ++j) {
            if (n2 & 1) { re[j] += pv[j] * so[j]; im[j] += pv[j] * se[j]; }
            else        { re[j] += pv[j] * se[j]; im[j] += pv[j] * so[j]; }
          }
        }
        const int g = src[s];
#pragma unroll
        for (int j = 0; j < NF; ++j) {
          if (j < nf) {                                // block-uniform
            const cf term = cmul(phc[j], {re[j], im[j]});
            const float* fl = flux + (size_t)(f0 + j) * fstride + s;
            if constexpr (BM == MF_PLAIN) {
              add_source<false>(term, [&](int i) { return fl[(size_t)i * S]; },
                                g, br, nullptr, 0, nullptr, 0, acc[j]);
            } else {
              // row f0 + j of the beam buffers (block-uniform offsets)
              const size_t fj = (size_t)(f0 + j);
              add_source<EJ>(
                  term, [&](int i) { return fl[(size_t)i * S]; }, g, br,
                  beam != nullptr ? beam + fj * bstride : nullptr, Nsta,
                  EJ ? ejones + fj * estride : nullptr, NE, acc[j]);
            }
          }
        }
      }
      sink.pass(ci, f0, nf, acc);
    }
    sink.cluster(ci);
  }
  sink.finish();
}

// The one place that unpacks the argument structs of this kernel family.
template <int NF, int BM, typename Sink>
__device__ __forceinline__ void shapelet_mf_kernel(
    const RowsUVW& rows, const ShapeletTabMF& tab, const Channels& ch,
    const BeamChannels& bm, const int* __restrict__ skip, int pass0,
    int pass1, Sink& sink) {
  const ShapeletTab& t = tab.t;
  shapelet_mf_body<NF, BM>(
      rows.u, rows.v, rows.w, rows.R, t.src, t.n0, t.beta, t.off, t.coef,
      t.cxi, t.sxi, t.cphi, t.sphi, t.psign, t.a, t.b, t.ceP, t.seP, t.ll,
      t.mm, t.nn1, t.rec, t.S, t.nmax, t.flux, t.r1, tab.entry_off, tab.M,
      ch.freqs, ch.F, ch.fdelta2, ch.tdelta, (size_t)ch.flux_stride, skip,
      BM != MF_PLAIN ? bm.beam : nullptr, BM == MF_EJ ? bm.ejones : nullptr,
      bm.pairs, bm.Nbase, bm.Ktot, bm.Nsta, BM == MF_EJ ? bm.NE : 0,
      (size_t)bm.T * bm.Ktot * bm.Nsta, (size_t)bm.T * bm.Ktot * bm.NE * 4,
      pass0, pass1, sink);
}

// out[f, ci, r, :] += C of every channel of the pass
template <int NF, bool EJ>
struct AddStoreSink {
  float2* out;                // [F, M, R, 4]
  int r, R, M;
  __device__ __forceinline__ void pass(int ci, int f0, int nf,
                                       const cf (&acc)[NF][4]) {
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      if (j < nf) {
        float2* o = out + (((size_t)(f0 + j) * M + ci) * R + r) * 4;
        put_coherency<EJ>(acc[j], [&](int i, cf c) { o[i] = cadd(o[i], c); });
      }
    }
  }
  __device__ __forceinline__ void cluster(int) {}
  __device__ __forceinline__ void finish() {}
};

// out[ci, r, :] += (sum over channels, in channel order) / F
template <int NF, bool EJ>
struct AddMeanSink {
  float2* out;                // [M, R, 4]
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
      o[i] = cadd(o[i], {m[i].x / nch, m[i].y / nch});
      m[i] = {0.f, 0.f};
    }
  }
  __device__ __forceinline__ void finish() {}
};

// out[f, r, :] -= sum over clusters of J_p C J_q^H
template <int NF, bool EJ>
struct SubModelSink {
  float2* out;                     // [F, R, 4], holds x - main model
  const float2* __restrict__ J;    // [Mt, N, 4]
  const int* __restrict__ chunk;   // chunk_tab + t, strided by T along ci
  int r, R, T, N;
  int p, q;                        // stations of the row, both >= 0
  int f0, nf;
  bool any;                        // a cluster was added (block-uniform)
  cf model[NF][4];
  __device__ __forceinline__ void pass(int ci, int, int,
                                       const cf (&acc)[NF][4]) {
    any = true;
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
    if (!any) return;
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      if (j < nf) {
        const size_t o = ((size_t)(f0 + j) * R + r) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) out[o + i] = csub(out[o + i], model[j][i]);
      }
    }
  }
};

// The three entries, each for every beam variant. Passes along blockIdx.z,
// except the mean, whose threads walk the passes themselves.
template <int NF, int BM>
__device__ __forceinline__ void shapelet_mf_entry(
    const RowsUVW& rows, const ShapeletTabMF& tab, const Channels& ch,
    const BeamChannels& bm, float2* out) {
  AddStoreSink<NF, BM == MF_EJ> sink = {
      out, (int)(blockIdx.x * blockDim.x + threadIdx.x), rows.R, tab.M};
  shapelet_mf_kernel<NF, BM>(rows, tab, ch, bm, nullptr, blockIdx.z,
                             blockIdx.z + 1, sink);
}

template <int NF, int BM>
__device__ __forceinline__ void shapelet_mean_entry(
    const RowsUVW& rows, const ShapeletTabMF& tab, const Channels& ch,
    const BeamChannels& bm, float2* out) {
  AddMeanSink<NF, BM == MF_EJ> sink = {
      out, (int)(blockIdx.x * blockDim.x + threadIdx.x), rows.R, ch.F,
      {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}}};
  shapelet_mf_kernel<NF, BM>(rows, tab, ch, bm, nullptr, 0,
                             (ch.F + NF - 1) / NF, sink);
}

// rows.R == res.T * res.Nbase (the launcher checks it); res.x is not read,
// out holds x minus the model of the main kernel
template <int NF, int BM>
__device__ __forceinline__ void shapelet_residual_entry(
    const RowsUVW& rows, const ShapeletTabMF& tab, const Channels& ch,
    const BeamChannels& bm, const ResidualArgs& res, float2* out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows.R) return;
  SubModelSink<NF, BM == MF_EJ> sink = {};
  sink.out = out;  sink.J = res.J;
  sink.r = r;  sink.R = rows.R;  sink.T = res.T;  sink.N = res.N;
  sink.f0 = blockIdx.z * NF;
  sink.nf = min(NF, ch.F - sink.f0);
  const int t = r / res.Nbase, b = r - t * res.Nbase;
  sink.p = res.pairs[2 * b];
  sink.q = res.pairs[2 * b + 1];
  if (sink.p < 0 || sink.q < 0) return;     // the row keeps x
  sink.chunk = res.chunk_tab + t;
  shapelet_mf_kernel<NF, BM>(rows, tab, ch, bm, res.skip, blockIdx.z,
                             blockIdx.z + 1, sink);
}

extern "C" __global__ SH_NO_PK void __launch_bounds__(128)
k_shapelet_coh_mf(RowsUVW rows, ShapeletTabMF tab, Channels ch, float2* out) {
  shapelet_mf_entry<SH_NF, MF_PLAIN>(rows, tab, ch, BeamChannels{}, out);
}

extern "C" __global__ SH_NO_PK void __launch_bounds__(128)
k_shapelet_coh_mean(RowsUVW rows, ShapeletTabMF tab, Channels ch,
                    float2* out) {
  shapelet_mean_entry<SH_NF, MF_PLAIN>(rows, tab, ch, BeamChannels{}, out);
}

extern "C" __global__ SH_NO_PK void __launch_bounds__(128)
k_shapelet_residual_mf(RowsUVW rows, ShapeletTabMF tab, Channels ch,
                       ResidualArgs res, float2* out) {
  shapelet_residual_entry<SH_NF, MF_PLAIN>(rows, tab, ch, BeamChannels{}, res,
                                           out);
}

// Scalar-gain variants: bm.beam, bm.pairs required.
extern "C" __global__ SH_NO_PK void __launch_bounds__(128)
k_shapelet_coh_mf_bm(RowsUVW rows, ShapeletTabMF tab, Channels ch,
                     BeamChannels bm, float2* out) {
  shapelet_mf_entry<SH_NF, MF_GAIN>(rows, tab, ch, bm, out);
}

extern "C" __global__ SH_NO_PK void __launch_bounds__(128)
k_shapelet_coh_mean_bm(RowsUVW rows, ShapeletTabMF tab, Channels ch,
                       BeamChannels bm, float2* out) {
  shapelet_mean_entry<SH_NF, MF_GAIN>(rows, tab, ch, bm, out);
}

extern "C" __global__ SH_NO_PK void __launch_bounds__(128)
k_shapelet_residual_mf_bm(RowsUVW rows, ShapeletTabMF tab, Channels ch,
                          BeamChannels bm, ResidualArgs res, float2* out) {
  shapelet_residual_entry<SH_NF, MF_GAIN>(rows, tab, ch, bm, res, out);
}

// E-Jones variants: bm.ejones, bm.pairs required; bm.beam may be null.
extern "C" __global__ SH_NO_PK void __launch_bounds__(128)
k_shapelet_coh_mf_ej(RowsUVW rows, ShapeletTabMF tab, Channels ch,
                     BeamChannels bm, float2* out) {
  shapelet_mf_entry<SH_NF_EJ, MF_EJ>(rows, tab, ch, bm, out);
}

extern "C" __global__ SH_NO_PK void __launch_bounds__(128)
k_shapelet_coh_mean_ej(RowsUVW rows, ShapeletTabMF tab, Channels ch,
                       BeamChannels bm, float2* out) {
  shapelet_mean_entry<SH_NF_EJ, MF_EJ>(rows, tab, ch, bm, out);
}

extern "C" __global__ SH_NO_PK void __launch_bounds__(128)
k_shapelet_residual_mf_ej(RowsUVW rows, ShapeletTabMF tab, Channels ch,
                          BeamChannels bm, ResidualArgs res, float2* out) {
  shapelet_residual_entry<SH_NF_EJ, MF_EJ>(rows, tab, ch, bm, res, out);
}
