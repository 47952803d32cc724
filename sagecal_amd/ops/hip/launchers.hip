// Kernel launch wrappers + kernels in ONE translation unit (no -fgpu-rdc
// cross-TU device linking needed).
#include "common.h"
#include "launchers.h"
#include "predict.hip"
#include "predict_mf.hip"
#include "jtj.hip"
#include "cholesky.hip"
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
}  // extern "C"
