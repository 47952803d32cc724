// The interface between launchers.hip (hipcc) and bindings.cpp (host
// compiler): every launch_* prototype and the argument structs of the two
// predict launchers. Both sides include this file, so a signature that
// changes on one side alone does not compile.
//
// The structs exist at the binding / launcher / kernel boundary only. A
// kernel takes them by value and unpacks each exactly once into the
// __restrict__ parameter list of its __device__ __forceinline__ body
// (predict.hip says why); nothing in a body reads a struct member.
#pragma once
#include <hip/hip_runtime.h>

// Baseline rows r = t*Nbase + b, uvw in seconds.
struct RowsUVW {
  const double *u, *v, *w;  // [R]
  int R;
};

// Per-source arrays of k_predict_coh (hip_host.GPUPack), K sources in M
// clusters; fluxes at the channel, shapelet sources zeroed.
struct SourceArrays {
  const double *ll, *mm, *nn1;
  const float *sI, *sQ, *sU, *sV;
  const float *eX, *eY, *eP;
  const float *cxi, *sxi, *cphi, *sphi;
  const float* r1;          // time-smear source-distance term
  const int* stype;
  const int* cluster_off;   // [M + 1]
  int M;
};

// Shapelet mode table of k_shapelet_coh, S entries; the pointers in
// hip_host.ShapeletTable.FIELDS order, then what changes per call.
struct ShapeletTab {
  const int *src, *cluster, *n0;
  const float* beta;
  const int* off;           // [S + 1]
  const float* coef;
  const float *cxi, *sxi, *cphi, *sphi, *psign, *a, *b, *ceP, *seP;
  const double *ll, *mm, *nn1;
  const float* rec;         // [2, nmax]
  int S, nmax;
  const float* flux;        // [4, S] I,Q,U,V at the channel
  const float* r1;          // [S]
};

struct Channel {
  double freq;
  double fdelta2;           // channel halfwidth [Hz]
  double tdelta;
};

// The F channels of the all-channels kernels (predict_mf.hip). With these
// the flux pointers of SourceArrays address channel 0 of [F, K] arrays
// whose rows lie flux_stride floats apart.
struct Channels {
  const double* freqs;      // [F], on the device
  int F;
  double fdelta2;           // channel halfwidth [Hz]
  double tdelta;
  long long flux_stride;
};

// What k_residual_mf takes besides the predict arguments.
struct ResidualArgs {
  const float2* x;          // [F, R, 4] data
  const float2* J;          // [Mt, N, 4] packed solutions
  const int* chunk_tab;     // [M, T] global chunk id, chunk_off[ci] added
  const int* pairs;         // [Nbase, 2]; a negative entry keeps x
  const int* skip;          // [M] non-zero: solved but not subtracted; or null
  int Nbase, T, N;
};

// Station beam of both predict kernels. beam null: no scalar gain; ejones
// null: the kernels without E-Jones run. pairs, Nbase and Ktot are read
// with either; Nsta strides beam, NE (1 or Nsta) strides ejones.
struct BeamArgs {
  const float* beam;        // [T, Ktot, Nsta] or null
  const int* pairs;         // [Nbase, 2]
  int Nbase, Ktot, Nsta;
  const float2* ejones;     // [T, Ktot, NE, 2, 2] or null
  int NE;
};

// Station beam of the all-channels kernels (predict_mf.hip), the buffers of
// BeamArgs with a leading channel axis: channel f reads row f. beam and
// ejones both null: the kernels without beam run. beam alone: the scalar
// gain kernels (_bm). ejones, with or without beam: the E-Jones kernels
// (_ej). pairs, Nbase, T and Ktot are read with either, and the rows are
// R == T * Nbase; Nsta strides beam, NE (1 or Nsta) strides ejones.
struct BeamChannels {
  const float* beam;        // [F, T, Ktot, Nsta] or null
  const float2* ejones;     // [F, T, Ktot, NE, 2, 2] or null
  const int* pairs;         // [Nbase, 2]
  int Nbase, T, Ktot, Nsta, NE;
};

extern "C" {

// out [M, R, 4]: written by launch_predict_coh, added into by
// launch_shapelet_coh. hipErrorInvalidValue: ejones without pairs or
// Nbase, or NE neither 1 nor Nsta.
hipError_t launch_predict_coh(RowsUVW rows, SourceArrays src, Channel ch,
                              BeamArgs bm, float2* out, hipStream_t stream);
hipError_t launch_shapelet_coh(RowsUVW rows, ShapeletTab tab, Channel ch,
                               BeamArgs bm, float2* out, hipStream_t stream);

// All channels in one launch, no shapelet sources (their fluxes arrive
// zeroed), with the station beam of bm when it holds one. Channels a thread
// carries per pass, without E-Jones and with:
#ifndef PREDICT_MF_NF
#define PREDICT_MF_NF 2
#endif
#ifndef PREDICT_MF_NF_EJ
#define PREDICT_MF_NF_EJ 1
#endif
// out [F, M, R, 4], or with mean != 0 the channel mean [M, R, 4].
// hipErrorInvalidValue: F < 1 or R < 1; with a beam or E-Jones: no pairs or
// Nbase, R != T * Nbase, Ktot or Nsta < 1, or (E-Jones) NE neither 1 nor
// Nsta.
hipError_t launch_predict_coh_mf(RowsUVW rows, SourceArrays src, Channels ch,
                                 BeamChannels bm, int mean, float2* out,
                                 hipStream_t stream);
// out [F, R, 4] = x - sum over clusters with skip == 0 of J_p C J_q^H.
// hipErrorInvalidValue: F < 1, R < 1, R != T * Nbase, or x, J, chunk_tab
// or pairs missing; with a beam or E-Jones what launch_predict_coh_mf
// refuses, or a bm that disagrees with res on pairs, Nbase or T.
hipError_t launch_residual_mf(RowsUVW rows, SourceArrays src, Channels ch,
                              BeamChannels bm, ResidualArgs res, float2* out,
                              hipStream_t stream);

hipError_t launch_array_beam(
    const double* elem, const int* nelem, const double* du,
    const unsigned char* below, int N, int Emax, int TK, double kf,
    float* gain, hipStream_t stream);
// tile and du_tile come together or not at all (single stage); D counts
// the dipoles of a tile and is ignored without them
hipError_t launch_station_beam(
    const double* elem, const int* nelem, const double* tile,
    const double* du, const double* du_tile, const unsigned char* below,
    const double* kfs, int N, int Emax, int D, int TK, int F, float* gain,
    hipStream_t stream);

// Dipole E-Jones E [F, D, 2, 2] of D directions (az, el fp64) at F
// frequencies: coef [F, 2, Nmodes] theta and phi rows, preamble [Nmodes],
// Nmodes = M(M+1)/2. hipErrorInvalidValue: M outside 1..ELEMENT_BEAM_MAX_M,
// F < 1 or beta not positive.
#define ELEMENT_BEAM_MAX_M 8
hipError_t launch_element_beam(
    const double* az, const double* el, const float2* coef,
    const float* preamble, int D, int F, int M, float beta, float2* E,
    hipStream_t stream);

hipError_t launch_jtj_accum(
    const float2* x, const float2* coh, const float2* J, const int* pairs,
    const int* chunk_tab, const int* pidx, const float* wts, int Nbase,
    int T, int N, int nseg, int Mt, float2* PD, float2* Pg, float* Pc,
    int* present, float2* D, float2* g, float2* Cx, float* cost, int npair,
    int grad_only, hipStream_t stream);
hipError_t launch_jtj_expand(
    const float2* D, const float2* g, const float2* Cx, const int* pairs,
    const int* pidx, int N, int npair, int Mt, float* JtJ, float* Jtr,
    hipStream_t stream);
hipError_t launch_model_cost(
    const float2* x, const float2* coh, const float2* J, const int* pairs,
    const int* chunk_tab, const float* wts, int Nbase, int T, int N,
    int nseg, int Mt, float* e2, float* cost, hipStream_t stream);
hipError_t launch_apply_jones(
    const float2* x, const float2* cohs, const float2* J, const int* pairs,
    const int* chunk_tab, int Nbase, int T, int N, int nseg, int M, int sub,
    float2* out, hipStream_t stream);

// dp = (JtJ + mu I)^-1 Jtr, one workgroup per problem (chol_solve) or the
// multi-workgroup kernel sequence (chol_mw); same contract, n a multiple of
// the block size, Lbuf 2*n*n floats per problem
hipError_t launch_chol_solve(
    const float* JtJ, const float* Jtr, const float* mu, int n, int batch,
    float* Lbuf, float* dp, int* info, hipStream_t stream);
hipError_t launch_chol_mw(
    const float* JtJ, const float* Jtr, const float* mu, int n, int batch,
    float* Lbuf, float* dp, int* info, hipStream_t stream);

}  // extern "C"
