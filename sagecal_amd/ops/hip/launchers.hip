// Kernel launch wrappers + kernels in ONE translation unit (no -fgpu-rdc
// cross-TU device linking needed).
#include "common.h"
#include "launchers.h"
#include "predict.hip"
#include "predict_mf.hip"
#include "shapelet_mf.hip"
#include "jtj.hip"
#include "lbfgs_mf.hip"
#include "joint_jtj.hip"
#include "rtr_tcg.hip"
#include "leverage.hip"
#include "normal_f64.hip"
#include "spd_inverse.hip"
#include "diffuse.hip"
#include "cholesky.hip"
#include "cholesky_blocked.hip"
#include "element_beam.hip"

// One thread per row in blocks of 128: the plain kernel, or with
// bm.ejones the _ej one, which reads pairs on every row. The two take the
// same arguments.
template <typename Args>
static hipError_t launch_rows(
    void (*plain)(RowsUVW, Args, Channel, BeamArgs, float2*),
    void (*ej)(RowsUVW, Args, Channel, BeamArgs, float2*), RowsUVW rows,
    Args args, Channel ch, BeamArgs bm, float2* out, hipStream_t stream) {
  const bool with_ej = bm.ejones != nullptr;
  if (with_ej && (bm.pairs == nullptr || bm.Nbase <= 0 ||
                  (bm.NE != 1 && bm.NE != bm.Nsta)))
    return hipErrorInvalidValue;
  const int tb = 128;
  hipLaunchKernelGGL(with_ej ? ej : plain, dim3((rows.R + tb - 1) / tb),
                     dim3(tb), 0, stream, rows, args, ch, bm, out);
  return hipGetLastError();
}

extern "C" {

hipError_t launch_predict_coh(RowsUVW rows, SourceArrays src, Channel ch,
                              BeamArgs bm, float2* out, hipStream_t stream) {
  return launch_rows(k_predict_coh, k_predict_coh_ej, rows, src, ch, bm, out,
                     stream);
}

hipError_t launch_shapelet_coh(RowsUVW rows, ShapeletTab tab, Channel ch,
                               BeamArgs bm, float2* out, hipStream_t stream) {
  if (tab.S <= 0 || rows.R <= 0) return hipSuccess;
  return launch_rows(k_shapelet_coh, k_shapelet_coh_ej, rows, tab, ch, bm,
                     out, stream);
}

// blocks of 128 rows; passes of nf channels along grid z except for the
// mean, whose threads walk the passes themselves
static bool mf_grid(int R, int F, int nf, bool z_passes, dim3* grid) {
  if (F < 1 || R < 1) return false;
  const long long gz = z_passes ? (F + nf - 1) / nf : 1;
  if (gz > 65535) return false;
  *grid = dim3((R + 127) / 128, 1, (unsigned)gz);
  return true;
}

// MF_PLAIN, MF_GAIN or MF_EJ for the buffers of bm, or -1 when the kernels
// would index them out of bounds
static int mf_beam_mode(const BeamChannels& bm, int R) {
  if (bm.beam == nullptr && bm.ejones == nullptr) return MF_PLAIN;
  if (bm.pairs == nullptr || bm.Nbase < 1 || bm.T < 1 || bm.Ktot < 1 ||
      bm.Nsta < 1 || (long long)bm.T * bm.Nbase != R)
    return -1;
  if (bm.ejones == nullptr) return MF_GAIN;
  return bm.NE == 1 || bm.NE == bm.Nsta ? MF_EJ : -1;
}

hipError_t launch_predict_coh_mf(RowsUVW rows, SourceArrays src, Channels ch,
                                 BeamChannels bm, int mean, float2* out,
                                 hipStream_t stream) {
  dim3 grid;
  const int mode = mf_beam_mode(bm, rows.R);
  if (mode < 0 || ch.freqs == nullptr ||
      !mf_grid(rows.R, ch.F, mode == MF_EJ ? MF_NF_EJ : MF_NF, !mean, &grid))
    return hipErrorInvalidValue;
  if (mode == MF_PLAIN)
    hipLaunchKernelGGL(mean ? k_predict_coh_mean : k_predict_coh_mf, grid,
                       dim3(128), 0, stream, rows, src, ch, out);
  else if (mode == MF_GAIN)
    hipLaunchKernelGGL(mean ? k_predict_coh_mean_bm : k_predict_coh_mf_bm,
                       grid, dim3(128), 0, stream, rows, src, ch, bm, out);
  else
    hipLaunchKernelGGL(mean ? k_predict_coh_mean_ej : k_predict_coh_mf_ej,
                       grid, dim3(128), 0, stream, rows, src, ch, bm, out);
  return hipGetLastError();
}

hipError_t launch_residual_mf(RowsUVW rows, SourceArrays src, Channels ch,
                              BeamChannels bm, ResidualArgs res, float2* out,
                              hipStream_t stream) {
  dim3 grid;
  const int mode = mf_beam_mode(bm, rows.R);
  if (mode < 0 || ch.freqs == nullptr ||
      !mf_grid(rows.R, ch.F, mode == MF_EJ ? MF_NF_EJ : MF_NF, true, &grid) ||
      res.x == nullptr || res.J == nullptr || res.chunk_tab == nullptr ||
      res.pairs == nullptr || res.Nbase < 1 || res.T < 1 || res.N < 1 ||
      (long long)res.T * res.Nbase != rows.R)
    return hipErrorInvalidValue;
  if (mode != MF_PLAIN && (bm.pairs != res.pairs || bm.Nbase != res.Nbase ||
                           bm.T != res.T))
    return hipErrorInvalidValue;
  if (mode == MF_PLAIN)
    hipLaunchKernelGGL(k_residual_mf, grid, dim3(128), 0, stream, rows, src,
                       ch, res, out);
  else if (mode == MF_GAIN)
    hipLaunchKernelGGL(k_residual_mf_bm, grid, dim3(128), 0, stream, rows,
                       src, ch, bm, res, out);
  else
    hipLaunchKernelGGL(k_residual_mf_ej, grid, dim3(128), 0, stream, rows,
                       src, ch, bm, res, out);
  return hipGetLastError();
}

static bool shapelet_tab_ok(const ShapeletTabMF& tab) {
  return tab.t.S >= 1 && tab.M >= 1 && tab.entry_off != nullptr &&
         tab.t.flux != nullptr && tab.t.r1 != nullptr;
}

hipError_t launch_shapelet_coh_mf(RowsUVW rows, ShapeletTabMF tab,
                                  Channels ch, BeamChannels bm, int mean,
                                  float2* out, hipStream_t stream) {
  dim3 grid;
  const int mode = mf_beam_mode(bm, rows.R);
  if (mode < 0 || ch.freqs == nullptr || !shapelet_tab_ok(tab) ||
      !mf_grid(rows.R, ch.F, mode == MF_EJ ? SH_NF_EJ : SH_NF, !mean, &grid))
    return hipErrorInvalidValue;
  if (mode == MF_PLAIN)
    hipLaunchKernelGGL(mean ? k_shapelet_coh_mean : k_shapelet_coh_mf, grid,
                       dim3(128), 0, stream, rows, tab, ch, out);
  else if (mode == MF_GAIN)
    hipLaunchKernelGGL(mean ? k_shapelet_coh_mean_bm : k_shapelet_coh_mf_bm,
                       grid, dim3(128), 0, stream, rows, tab, ch, bm, out);
  else
    hipLaunchKernelGGL(mean ? k_shapelet_coh_mean_ej : k_shapelet_coh_mf_ej,
                       grid, dim3(128), 0, stream, rows, tab, ch, bm, out);
  return hipGetLastError();
}

hipError_t launch_shapelet_residual_mf(RowsUVW rows, ShapeletTabMF tab,
                                       Channels ch, BeamChannels bm,
                                       ResidualArgs res, float2* out,
                                       hipStream_t stream) {
  dim3 grid;
  const int mode = mf_beam_mode(bm, rows.R);
  if (mode < 0 || ch.freqs == nullptr || !shapelet_tab_ok(tab) ||
      !mf_grid(rows.R, ch.F, mode == MF_EJ ? SH_NF_EJ : SH_NF, true, &grid) ||
      res.J == nullptr || res.chunk_tab == nullptr || res.pairs == nullptr ||
      res.Nbase < 1 || res.T < 1 || res.N < 1 ||
      (long long)res.T * res.Nbase != rows.R)
    return hipErrorInvalidValue;
  if (mode != MF_PLAIN && (bm.pairs != res.pairs || bm.Nbase != res.Nbase ||
                           bm.T != res.T))
    return hipErrorInvalidValue;
  if (mode == MF_PLAIN)
    hipLaunchKernelGGL(k_shapelet_residual_mf, grid, dim3(128), 0, stream,
                       rows, tab, ch, res, out);
  else if (mode == MF_GAIN)
    hipLaunchKernelGGL(k_shapelet_residual_mf_bm, grid, dim3(128), 0, stream,
                       rows, tab, ch, bm, res, out);
  else
    hipLaunchKernelGGL(k_shapelet_residual_mf_ej, grid, dim3(128), 0, stream,
                       rows, tab, ch, bm, res, out);
  return hipGetLastError();
}

hipError_t launch_array_beam(
    const double* elem, const int* nelem, const double* du,
    const unsigned char* below, int N, int Emax, int TK, double kf,
    float* gain, hipStream_t stream) {
  if (N <= 0 || TK <= 0) return hipSuccess;
  if (Emax <= 0) return hipErrorInvalidValue;
  const int tb = 256;
  hipLaunchKernelGGL(k_array_beam,
      dim3((TK + tb - 1) / tb, (N + AB_NSTA - 1) / AB_NSTA), dim3(tb), 0,
      stream, elem, nelem, du, below, N, Emax, TK, kf, gain);
  return hipGetLastError();
}

// tile and du_tile come together or not at all (single stage); D counts
// the dipoles of a tile and is ignored without them
hipError_t launch_station_beam(
    const double* elem, const int* nelem, const double* tile,
    const double* du, const double* du_tile, const unsigned char* below,
    const double* kfs, int N, int Emax, int D, int TK, int F, float* gain,
    hipStream_t stream) {
  if (N <= 0 || TK <= 0 || F <= 0) return hipSuccess;
  if (Emax <= 0 || (tile == nullptr) != (du_tile == nullptr))
    return hipErrorInvalidValue;
  if (tile != nullptr && (D < 1 || D > SB_DMAX)) return hipErrorInvalidValue;
  const int tb = 256;
  const long long gy = (N + SB_NSTA - 1) / SB_NSTA;
  const long long gz = (F + SB_NF - 1) / SB_NF;
  if (gy > 65535 || gz > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_station_beam,
      dim3((TK + tb - 1) / tb, (unsigned)gy, (unsigned)gz), dim3(tb), 0,
      stream, elem, nelem, tile, du, du_tile, below, kfs, N, Emax, D, TK, F,
      gain);
  return hipGetLastError();
}

// coef [F, 2, M(M+1)/2], preamble [M(M+1)/2], E [F, D, 2, 2]; the kernel
// unrolls its mode loops to EB_MAX_M and divides by beta
hipError_t launch_element_beam(
    const double* az, const double* el, const float2* coef,
    const float* preamble, int D, int F, int M, float beta, float2* E,
    hipStream_t stream) {
  if (M < 1 || M > EB_MAX_M || F < 1 || D < 0 || !(beta > 0.f))
    return hipErrorInvalidValue;
  if (D == 0) return hipSuccess;
  hipLaunchKernelGGL(k_element_beam, dim3((D + EB_TB - 1) / EB_TB),
                     dim3(EB_TB), 0, stream, az, el, coef, preamble, D, F, M,
                     beta, E);
  return hipGetLastError();
}

hipError_t launch_jtj_accum(
    const float2* x, const float2* coh, const float2* J, const int* pairs,
    const int* chunk_tab, const int* pidx, const float* wts, int Nbase,
    int T, int N, int nseg, int Mt, float2* PD, float2* Pg, float* Pc,
    int* present, float2* D, float2* g, float2* Cx, float* cost, int npair,
    int grad_only, hipStream_t stream) {
  // store pass (one slot per chunk and pair), then the per-station and
  // per-chunk sum pass; D, g, cost and present arrive zeroed
  hipLaunchKernelGGL(k_jtj_accum, dim3(Nbase, nseg), dim3(64), 0, stream,
      x, coh, J, pairs, chunk_tab, wts, Nbase, T, N, PD, Pg, Cx, Pc, present,
      npair, grad_only);
  hipLaunchKernelGGL(k_jtj_reduce, dim3(N + 1, Mt), dim3(64), 0, stream,
      PD, Pg, Pc, present, pairs, pidx, N, Nbase, npair, grad_only, D, g,
      cost);
  return hipGetLastError();
}

// residual pass, gradient pass, fixed-order reduction (lbfgs_mf.hip)
hipError_t launch_lbfgs_mf(LbfgsMfArgs a, float2* sres, float2* slots,
                           float* cpart, float* cost, float* grad,
                           hipStream_t stream) {
  if (a.F < 1 || a.M < 1 || a.T < 1 || a.Nbase < 1 || a.N < 1 || a.Mt < 1 ||
      a.E < 1 || a.F > 65535)
    return hipErrorInvalidValue;
  const long long R = (long long)a.T * a.Nbase;
  const long long nblk = (R + LBFGS_MF_TB - 1) / LBFGS_MF_TB;
  const long long tiles = (a.Nbase + LBFGS_MF_TB - 1) / LBFGS_MF_TB;
  const size_t lds = (size_t)a.N * 4 * sizeof(float2);
  if (nblk >= (1LL << 31) || tiles > 65535 || lds > 65536 ||
      (long long)a.Mt * a.N + 1 >= (1LL << 31))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_lbfgs_mf_res, dim3((unsigned)nblk, a.F),
                     dim3(LBFGS_MF_TB), 0, stream, a, sres, cpart);
  hipLaunchKernelGGL(k_lbfgs_mf_grad, dim3(a.E, (unsigned)tiles),
                     dim3(LBFGS_MF_TB), lds, stream, a, sres, slots);
  hipLaunchKernelGGL(k_lbfgs_mf_reduce, dim3((unsigned)(a.Mt * a.N + 1)),
                     dim3(WAVE), 0, stream, a, slots, cpart, nblk * a.F, grad,
                     cost);
  return hipGetLastError();
}

// LDS of k_joint_gram and k_joint_cost: z, res and the 2 M Jones in play
static bool joint_shape_ok(const JointJtjArgs& a, size_t* lds) {
  if (a.M < 1 || a.T < 1 || a.Nbase < 1 || a.N < 1 || a.Mt < 1 || a.E < 1 ||
      a.nbin < 1 || 2 * a.M > JOINT_JTJ_TB)
    return false;
  *lds = ((size_t)JOINT_JTJ_TT * a.M * 8 + JOINT_JTJ_TT * 4 +
          (size_t)2 * a.M * 4) * sizeof(float2);
  return *lds <= 65536;
}

// per-pair pass, then the fixed-order per-station reduction (joint_jtj.hip)
hipError_t launch_joint_jtj(JointJtjArgs a, float2* PE, float2* PG, float* PC,
                            float* H, float* g, float* cost,
                            hipStream_t stream) {
  size_t lds;
  if (!joint_shape_ok(a, &lds) || a.D < 1 || a.G < 1 || a.ld < 8)
    return hipErrorInvalidValue;
  const long long nred = (long long)a.N * (a.D + a.G) + a.nbin;
  if (nred >= (1LL << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_joint_gram, dim3(a.Nbase), dim3(JOINT_JTJ_TB), lds,
                     stream, a, H, PE, PG, PC);
  hipLaunchKernelGGL(k_joint_reduce, dim3((unsigned)nred), dim3(WAVE), 0,
                     stream, a, PE, PG, PC, H, g, cost);
  return hipGetLastError();
}

hipError_t launch_joint_cost(JointJtjArgs a, float* PC, float* cost,
                             hipStream_t stream) {
  size_t lds;
  if (!joint_shape_ok(a, &lds)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_joint_cost, dim3(a.Nbase), dim3(JOINT_JTJ_TB), lds,
                     stream, a, PC);
  hipLaunchKernelGGL(k_joint_cost_reduce, dim3(a.nbin), dim3(WAVE), 0, stream,
                     a, PC, cost);
  return hipGetLastError();
}

// one workgroup per chunk; LDS holds v, Hv and iw (rtr_tcg.hip)
hipError_t launch_rtr_tcg(RtrTcgArgs a, float2* g, float2* eta, float2* Heta,
                          float* stats, hipStream_t stream) {
  if (a.n < 1 || a.N < 2 || 8 * (long long)a.N > RTR_TCG_MAXP || a.maxit < 0)
    return hipErrorInvalidValue;
  const size_t lds = (size_t)(2 * 8 * a.N + a.N) * sizeof(float);
  hipLaunchKernelGGL(k_rtr_tcg, dim3(a.n), dim3(RTR_TCG_TB), lds, stream, a,
                     g, eta, Heta, stats);
  return hipGetLastError();
}

// one workgroup per (tile of WAVE pairs, piece); static LDS (leverage.hip)
hipError_t launch_leverage(LeverageArgs a, double* lev, hipStream_t stream) {
  if (a.M < 1 || a.T < 1 || a.Nbase < 1 || a.N < 1 || a.Mt < 1 || a.E < 1 ||
      a.E > 65535 || a.cohs == nullptr || a.J == nullptr ||
      a.Hinv == nullptr || a.pairs == nullptr || a.pieces == nullptr ||
      lev == nullptr || (long long)a.T * a.Nbase * a.M > (1LL << 40))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_leverage, dim3((a.Nbase + WAVE - 1) / WAVE, a.E),
                     dim3(LEVERAGE_TB), 0, stream, a, lev);
  return hipGetLastError();
}

// one workgroup per (tile of WAVE pairs, piece), then one per (tile pair of
// 8 x 8 stations, chunk); static LDS (normal_f64.hip)
hipError_t launch_normal_f64(NormalF64Args a, double* part, double* JtJ,
                             hipStream_t stream) {
  if (a.M < 1 || a.T < 1 || a.Nbase < 1 || a.N < 1 || a.N > 8192 ||
      a.Mt < 1 || a.Mt > 65535 || a.E < 1 || a.E > 65535 ||
      a.cohs == nullptr || a.J == nullptr || a.pairs == nullptr ||
      a.pieces == nullptr || a.piece_off == nullptr || a.pidx == nullptr ||
      a.sta_off == nullptr || a.sta_ent == nullptr || part == nullptr ||
      JtJ == nullptr || (long long)a.T * a.Nbase * a.M > (1LL << 40))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_normal_accum, dim3((a.Nbase + WAVE - 1) / WAVE, a.E),
                     dim3(NORMAL_F64_TB), 0, stream, a, part);
  const int nt = (a.N + 7) / 8;
  hipLaunchKernelGGL(k_normal_expand, dim3(nt * (nt + 1) / 2, a.Mt),
                     dim3(NORMAL_F64_TB), 0, stream, a, part, JtJ);
  return hipGetLastError();
}

// the per-station operands (a workgroup per station and row of C Z^H, one
// more per station for Z's half), then a workgroup per pair (diffuse.hip)
hipError_t launch_diffuse(DiffuseArgs a, float2* out, hipStream_t stream) {
  if (a.T < 1 || a.Nbase < 1 || a.N < 1 || a.N > 65535 || a.Gz < 1 ||
      a.Gz > DIFFUSE_MAX_GZ || a.Gc < 1 ||
      a.Gc + 2 * a.Gz - 2 > DIFFUSE_MAX_N2 || a.u == nullptr ||
      a.v == nullptr || a.w == nullptr || a.pairs == nullptr ||
      a.Z == nullptr || a.C == nullptr || a.T1 == nullptr ||
      a.T2 == nullptr || a.A == nullptr || a.B == nullptr || out == nullptr)
    return hipErrorInvalidValue;
  const int n1 = a.Gc + a.Gz - 1;
  hipLaunchKernelGGL(k_diffuse_station, dim3(a.N, n1 + 1), dim3(DIF_TB), 0,
                     stream, a);
  hipLaunchKernelGGL(k_diffuse_pair, dim3(a.Nbase), dim3(DIF_TB), 0, stream,
                     a, out);
  return hipGetLastError();
}

// potrf (two launches per 32 columns, the first pair reading A), trtri (one
// per block column), lauum; one workgroup per 32 x 32 block
// (spd_inverse.hip)
hipError_t launch_spd_inverse(SpdInverseArgs a, double* X,
                              hipStream_t stream) {
  if (a.Mt < 1 || a.n < 8 || a.n > SPD_INVERSE_MAXN || a.n % 8 != 0 ||
      a.A == nullptr || a.mu == nullptr || a.W == nullptr ||
      a.D == nullptr || a.info == nullptr || X == nullptr ||
      (a.mu_stride != 0 && a.mu_stride != 1))
    return hipErrorInvalidValue;
  const int nt = (a.n + SPD_NB - 1) / SPD_NB;
  if ((long long)a.Mt * (nt * (nt + 1) / 2) > 0x7fffffffLL)
    return hipErrorInvalidValue;
  const dim3 tb(SPD_TB);
  for (int kb = 0; kb < nt; ++kb) {
    const int k = kb * SPD_NB, nb = nt - kb - 1;
    const dim3 gp(a.Mt * (nb > 0 ? nb : 1));
    const int ntiles = nb * (nb + 1) / 2;
    const dim3 gs(a.Mt * ntiles);
    if (kb > 0) {
      hipLaunchKernelGGL(k_spdinv_panel, gp, tb, 0, stream, a, k, nb);
      if (nb > 0)
        hipLaunchKernelGGL(k_spdinv_syrk, gs, tb, 0, stream, a, k, ntiles);
    } else if (a.a_f64) {
      hipLaunchKernelGGL(k_spdinv_panel_f64, gp, tb, 0, stream, a, k, nb);
      if (nb > 0)
        hipLaunchKernelGGL(k_spdinv_syrk_f64, gs, tb, 0, stream, a, k,
                           ntiles);
    } else {
      hipLaunchKernelGGL(k_spdinv_panel_f32, gp, tb, 0, stream, a, k, nb);
      if (nb > 0)
        hipLaunchKernelGGL(k_spdinv_syrk_f32, gs, tb, 0, stream, a, k,
                           ntiles);
    }
  }
  for (int I = 1; I < nt; ++I)
    hipLaunchKernelGGL(k_spdinv_trtri, dim3(a.Mt * I), tb, 0, stream, a, I);
  hipLaunchKernelGGL(k_spdinv_lauum, dim3(a.Mt * (nt * (nt + 1) / 2)), tb, 0,
                     stream, a, X);
  return hipGetLastError();
}

hipError_t launch_jtj_expand(
    const float2* D, const float2* g, const float2* Cx, const int* pairs,
    const int* pidx, int N, int npair, int Mt, float* JtJ, float* Jtr,
    hipStream_t stream) {
  hipLaunchKernelGGL(k_jtj_expand, dim3(N, N, Mt), dim3(64), 0, stream,
      D, g, Cx, pairs, pidx, N, npair, JtJ, Jtr);
  return hipGetLastError();
}

hipError_t launch_model_cost(
    const float2* x, const float2* coh, const float2* J, const int* pairs,
    const int* chunk_tab, const float* wts, int Nbase, int T, int N,
    int nseg, int Mt, float* e2, float* cost, hipStream_t stream) {
  const long long B = (long long)nseg * T * Nbase;
  const int tb = 256;
  const int nb = (int)((B + tb - 1) / tb);
  hipLaunchKernelGGL(k_model_cost, dim3(nb), dim3(tb), 0, stream,
      x, coh, J, pairs, chunk_tab, wts, Nbase, T, N, nseg, e2);
  // e2 holds B per-row costs followed by nseg*T per-slot sums
  float* slot_cost = e2 + B;
  hipLaunchKernelGGL(k_slot_cost, dim3(nseg * T), dim3(tb), 0, stream,
      e2, Nbase, slot_cost);
  hipLaunchKernelGGL(k_chunk_cost, dim3(Mt), dim3(tb), 0, stream,
      slot_cost, chunk_tab, nseg * T, cost);
  return hipGetLastError();
}

hipError_t launch_apply_jones(
    const float2* x, const float2* cohs, const float2* J, const int* pairs,
    const int* chunk_tab, int Nbase, int T, int N, int nseg, int M, int sub,
    float2* out, hipStream_t stream) {
  const long long B = (long long)nseg * T * Nbase;
  const int tb = 256;
  const int nb = (int)((B + tb - 1) / tb);
  hipLaunchKernelGGL(k_apply_jones, dim3(nb), dim3(tb), 0, stream,
      x, cohs, J, pairs, chunk_tab, Nbase, T, N, nseg, M, sub, out);
  return hipGetLastError();
}

// shape contract shared by both Cholesky launchers (see cholesky.hip):
// violated, the kernels would run float4 traffic out of bounds or ask for
// more LDS than a CU has
static bool chol_shape_ok(int n, int batch, int maxn) {
  return n > 0 && n % NB == 0 && n <= maxn && batch > 0;
}

hipError_t launch_chol_solve(
    const float* JtJ, const float* Jtr, const float* mu, int n, int batch,
    float* Lbuf, float* dp, int* info, hipStream_t stream) {
  if (!chol_shape_ok(n, batch, MAXN_CHOL)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_chol_solve, dim3(batch), dim3(NTH),
      chol_solve_lds_bytes(n), stream, JtJ, Jtr, mu, n, Lbuf, dp, info);
  return hipGetLastError();
}

// multi-workgroup right-looking variant: kernel sequence on one stream
// (graph-capturable). See cholesky.hip for the rationale.
hipError_t launch_chol_mw(
    const float* JtJ, const float* Jtr, const float* mu, int n, int batch,
    float* Lbuf, float* dp, int* info, hipStream_t stream) {
  if (!chol_shape_ok(n, batch, MAXN_CHOL_MW)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cholmw_init, dim3(batch, INIT_SLICES), dim3(NTH), 0,
      stream, JtJ, Jtr, mu, n, Lbuf, dp);
  // n <= PANEL_CAP: the single-pass panel kernel; larger n: the
  // chunked-panel variant (row passes through LDS)
  const size_t shmem = cholmw_panel_lds_bytes(n);
  for (int k = 0; k < n; k += NB) {
    if (n <= PANEL_CAP) {
      hipLaunchKernelGGL(k_cholmw_panel, dim3(batch), dim3(NTH), shmem,
          stream, n, k, Lbuf, dp, info);
    } else {
      hipLaunchKernelGGL(k_cholmw_panel_big, dim3(batch), dim3(NTH),
          shmem, stream, n, k, Lbuf, dp, info);
    }
    const int tcnt = (n - k - NB) / NB;
    const int ntiles = tcnt * (tcnt + 1) / 2;
    if (ntiles > 0) {
      hipLaunchKernelGGL(k_cholmw_syrk, dim3(batch * ntiles), dim3(64), 0,
          stream, n, k, ntiles, Lbuf);
    }
  }
  hipLaunchKernelGGL(k_cholmw_subst, dim3(batch), dim3(NTH), 0, stream,
      n, Lbuf, dp, info);
  return hipGetLastError();
}

// blocked variant for large n: outer blocks of XB columns, three launches
// per block (see cholesky_blocked.hip); init and the backward pass are the
// mw kernels
hipError_t launch_chol_blocked(
    const float* JtJ, const float* Jtr, const float* mu, int n, int batch,
    float* Lbuf, float* dp, int* info, hipStream_t stream) {
  if (!chol_shape_ok(n, batch, MAXN_CHOL_XL)) return hipErrorInvalidValue;
  const long long tmax = (n + XB - 1) / XB;
  if (batch * (tmax * (tmax + 1) / 2) > 0x7fffffffLL)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cholmw_init, dim3(batch, INIT_SLICES), dim3(NTH), 0,
      stream, JtJ, Jtr, mu, n, Lbuf, dp);
  for (int k = 0; k < n; k += XB) {
    hipLaunchKernelGGL(k_cholxl_diag, dim3(batch), dim3(NTH),
        cholxl_diag_lds_bytes(), stream, n, k, Lbuf, dp, info);
    const int rest = n - k - XB;          // rows below the block
    if (rest <= 0) break;
    const int nstrips = (rest + XS - 1) / XS;
    hipLaunchKernelGGL(k_cholxl_trsm, dim3(batch * nstrips), dim3(NTH),
        cholxl_trsm_lds_bytes(), stream, n, k, nstrips, Lbuf, dp);
    const int tcnt = (rest + XB - 1) / XB;
    const int ntiles = tcnt * (tcnt + 1) / 2;
    hipLaunchKernelGGL(k_cholxl_syrk, dim3(batch * ntiles), dim3(XTH), 0,
        stream, n, k, ntiles, Lbuf);
  }
  hipLaunchKernelGGL(k_cholmw_subst, dim3(batch), dim3(NTH), 0, stream,
      n, Lbuf, dp, info);
  return hipGetLastError();
}
}  // extern "C"
