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

// Shapelet mode table of k_shapelet_coh, S entries; the fields the binding
// looks up by name in hip_host.ShapeletTable.record, then what changes per
// call.
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

// Shapelet mode table of the all-channels kernels (shapelet_mf.hip): the
// table above, its `cluster` unread, with t.flux the [F, 4, S] stack of the
// channels' fluxes (rows Channels.flux_stride floats apart) and t.r1 [S],
// and the entries of cluster ci at entry_off[ci] <= s < entry_off[ci + 1].
struct ShapeletTabMF {
  ShapeletTab t;
  const int* entry_off;     // [M + 1]
  int M;
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

// The multi-channel LBFGS cost and gradient (lbfgs_mf.hip). Rows
// r = t*Nbase + b, R = T*Nbase. The host guarantees pair entries below N
// (negative: the row adds nothing), chunk ids in 0..Mt-1, and the three
// index tables as hip_host._lbfgs_tables builds them.
struct LbfgsMfArgs {
  const float2* xs;         // [F, R, 4] data
  const float2* cohs;       // [F, M, R, 4] coherencies
  const float2* J;          // [Mt, N, 4] packed solutions
  const int* pairs;         // [Nbase, 2]
  const int* chunk_tab;     // [M, T] global chunk id, chunk_off[ci] added
  const int* ext;           // [E, 4] extents (ci, c, t0, t1), sorted by c:
                            // timeslots t0 <= t < t1 of cluster ci, chunk c
  const int* ext_off;       // [Mt + 1] extents of chunk c: ext_off[c] <= e
                            // < ext_off[c + 1]
  const int* sta_off;       // [N + 1] entries of station s in sta_ent
  const int* sta_ent;       // 2*b + side for every unflagged pair b and
                            // side (0: p, 1: q), sorted by station, then b
  int F, M, T, Nbase, N, Mt, E;
  float nu;                 // robust nu; <= 0: Gaussian cost
};

// The joint cross-cluster normal equations (joint_jtj.hip). Rows
// r = t*Nbase + b, R = T*Nbase. The host guarantees pair entries below N
// (negative: the pair adds nothing), chunk ids in 0..Mt-1 and the tables
// as hip_host._joint_tables and hip_host._lbfgs_stations build them.
struct JointJtjArgs {
  const float2* x;          // [R, 4] data
  const float2* cohs;       // [M, R, 4] coherencies
  const float2* J;          // [Mt, N, 4] packed solutions
  const float* wts;         // [R] row weights >= 0, or null
  const int* pairs;         // [Nbase, 2]
  const int* chunk_tab;     // [M, T] global chunk id, chunk_off[ci] added
  const int* pieces;        // [E, 2] timeslots t0 <= t < t1, at most
                            // JOINT_JTJ_TT of them, every cluster's chunk
                            // id constant inside; in time order
  const int* etab;          // [E, M(M+1)/2] 2*slot + first, per piece and
                            // (ci <= cj) in row-major triangle order
  const int* gtab;          // [E, M] 2*gslot + first, per piece and cluster
  const int* cbin;          // [E] cost bin of the piece
  const int* sdst;          // [D, 2] chunks (c_i, c_j) of slot
  const int* gdst;          // [G] chunk of gslot
  const int* cpos;          // [Mt, 2] (block, position in block) of chunk
  const int* sta_off;       // [N + 1] entries of station s in sta_ent
  const int* sta_ent;       // 2*b + side, as in LbfgsMfArgs
  int M, T, Nbase, N, Mt, E, D, G, nbin;
  long long ld;             // rows of one block of H: 8 N (chunks per block)
};

// The RTR truncated-CG inner solve (rtr_tcg.hip), one workgroup per chunk.
// P = 8 N parameters per chunk in reference.vecR order.
struct RtrTcgArgs {
  const float* JtJ;         // [n, P, P], read as symmetric
  const float* Jtr;         // [n, P]
  const float2* J;          // [n, N, 4]
  const float* iw;          // [N] per-station gradient scale
  const float* delta;       // [n] trust-region radius
  int n, N, maxit;
  float kappa;
};

// The influence-map leverage (leverage.hip). Rows r = t*Nbase + b,
// R = T*Nbase. The host guarantees pair entries below N (negative: the row
// gets 0), chunk ids in 0..Mt-1 and pieces as hip_host._lbfgs_extents
// builds them from chunk_tab [M, T].
struct LeverageArgs {
  const float2* cohs;       // [M, R, 4] coherencies
  const float2* J;          // [Mt, N, 4] packed solutions
  const double* Hinv;       // [Mt, 8N, 8N] inverse of the damped JtJ
  const double* wts;        // [R] row weights, or null
  const int* pairs;         // [Nbase, 2]
  const int* pieces;        // [E, 4] (ci, c, t0, t1): timeslots t0 <= t < t1
                            // of cluster ci, all of global chunk c
  int M, T, Nbase, N, Mt, E;
};

// The float64 normal matrices of the influence map (normal_f64.hip). Rows
// r = t*Nbase + b, R = T*Nbase. The host guarantees pair entries below N,
// chunk ids in 0..Mt-1, pieces and piece_off as hip_host._lbfgs_extents
// builds them (sorted by chunk), sta_off and sta_ent as
// hip_host._lbfgs_stations does, and pidx from hip_host._normal_pair_index.
// cohs, J and pieces 16-byte aligned.
struct NormalF64Args {
  const float2* cohs;       // [M, R, 4] coherencies
  const float2* J;          // [Mt, N, 4] packed solutions
  const float* wts;         // [R] row weights, or null
  const int* pairs;         // [Nbase, 2]; a negative entry: the pair adds
                            // nothing
  const int* pieces;        // [E, 4] (ci, c, t0, t1): timeslots t0 <= t < t1
                            // of cluster ci, all of global chunk c
  const int* piece_off;     // [Mt + 1] first piece of each chunk
  const int* pidx;          // [N, N]: 2 b for pair b stored as (row, col),
                            // 2 b + 1 as (col, row), -1 for none
  const int* sta_off;       // [N + 1] a station's entries in sta_ent
  const int* sta_ent;       // 2 b + side, by station, then by entry
  int M, T, Nbase, N, Mt, E;
};

// The float64 inverse of damped SPD matrices (spd_inverse.hip), n a multiple
// of 8 and nt = ceil(n / 32) blocks a side. All pointers 16-byte aligned.
struct SpdInverseArgs {
  const void* A;            // [Mt, n, n] float32 or float64 (a_f64); the
                            // lower triangle is read, nothing is written
  const double* mu;         // [1] or [Mt], added to the diagonal
  double* W;                // scratch [Mt, n, n]
  double* D;                // scratch [Mt, nt, 2, 32, 32]
  int* info;                // [Mt], arrives zeroed
  int Mt, n;
  int a_f64;                // non-zero: A is float64
  int mu_stride;            // 0: one mu for all; 1: one per matrix
};

// The diffuse-cluster predict with the spatial model (diffuse.hip). Rows
// r = t*Nbase + b, R = T*Nbase; n1 = Gc + Gz - 1, n2 = Gz + n1 - 1. The host
// guarantees pair entries below N (negative: the row gets zeros). All
// pointers 16-byte aligned.
struct DiffuseArgs {
  const double *u, *v, *w;  // [R] seconds
  const int* pairs;         // [Nbase, 2]
  const double2* Z;         // [N, Gz*Gz, 4] station series
  const double2* C;         // [Gc*Gc, 4] sky series
  const double* T1;         // [n1, Gc, Gz] product tensor of C x Z^H
  const double* T2;         // [n2, Gz, n1] product tensor of Z x (C Z^H)
  double* A;                // scratch [N, RA, Kp], RA = DIFFUSE_PAD16(2 n2),
                            // Kp = DIFFUSE_PAD16(4 n1 Gz)
  double* B;                // scratch [N, RB, Kp], RB = DIFFUSE_PAD16(4 n2)
  int T, Nbase, N, Gz, Gc;
  double g2;                // scale of the product series
  double ll, mm, nn1;       // direction of the cluster
  double freq, fdelta2;     // channel [Hz] and its halfwidth
};

extern "C" {

// The supported range of launch_diffuse: the pair kernel keeps H_pq, n2 x n2
// 2x2 complex64 blocks, in 32 KB of LDS, over the 27 KB in which it staged
// the operands of the product, and covers the 2 n2 rows of that product with
// the four 16-row tiles of its four waves; the station kernel's LDS holds
// Gz x Gc <= DIFFUSE_MAX_GZ x DIFFUSE_MAX_N2 blocks.
#define DIFFUSE_MAX_GZ 4
#define DIFFUSE_MAX_N2 32
#define DIFFUSE_PAD16(x) (((x) + 15) / 16 * 16)
// out [R, 4] complex64, fully written; the scratch is fully written before
// it is read. hipErrorInvalidValue: a dimension < 1, Gz > DIFFUSE_MAX_GZ,
// n2 > DIFFUSE_MAX_N2, N > 65535 or a null pointer.
hipError_t launch_diffuse(DiffuseArgs a, float2* out, hipStream_t stream);

// The largest n of launch_spd_inverse.
#define SPD_INVERSE_MAXN 1024
// X [Mt, n, n] = (A + mu I)^-1, both triangles written, X == X^T to the
// bit. A non-positive pivot sets info[matrix] and fills that matrix of X
// with NaN. Scratch contents are unspecified on entry and exit.
// hipErrorInvalidValue: Mt < 1, n < 8, n > SPD_INVERSE_MAXN, n not a
// multiple of 8, a null pointer, or mu_stride neither 0 nor 1.
hipError_t launch_spd_inverse(SpdInverseArgs a, double* X,
                              hipStream_t stream);

// Threads per workgroup of k_leverage; a workgroup serves WAVE pairs.
#define LEVERAGE_TB 256
// lev [M, R] float64, fully written when the pieces cover every (cluster,
// timeslot). hipErrorInvalidValue: a dimension < 1, a null table, E > 65535
// or R * M beyond 2^40.
hipError_t launch_leverage(LeverageArgs a, double* lev, hipStream_t stream);

// Threads per workgroup of k_normal_accum (WAVE pairs) and k_normal_expand
// (a tile of 8 x 8 stations).
#define NORMAL_F64_TB 256
// Doubles per (piece, pair) of the scratch of launch_normal_f64.
#define NORMAL_F64_NV 40
// JtJ [Mt, 8N, 8N] float64, fully written, blocks of absent pairs and of
// chunks without a piece zero. Scratch part [E, Nbase, NORMAL_F64_NV],
// contents unspecified on entry and exit. hipErrorInvalidValue: a dimension
// < 1, a null table, E or Mt > 65535, N > 8192 or R * M beyond 2^40.
hipError_t launch_normal_f64(NormalF64Args a, double* part, double* JtJ,
                             hipStream_t stream);

// Threads per workgroup of k_rtr_tcg and the most parameters of a chunk:
// a thread owns one float4 of every vector.
#define RTR_TCG_TB 1024
#define RTR_TCG_MAXP 4096
// g, eta, Heta [n, N, 4] and stats [n, 4] (<g,g>, <g,eta>, <eta,Heta>, CG
// iterations entered), all fully written. hipErrorInvalidValue: n < 1,
// N < 2, 8 N > RTR_TCG_MAXP or maxit < 0.
hipError_t launch_rtr_tcg(RtrTcgArgs a, float2* g, float2* eta, float2* Heta,
                          float* stats, hipStream_t stream);

// Threads per workgroup of k_joint_gram, and the most timeslots of one of
// its pieces (the time tile z is staged for in LDS).
#define JOINT_JTJ_TB 128
#define JOINT_JTJ_TT 32
// H [nblk, ld, ld] and g [nblk, ld] arrive zeroed and get every
// structurally non-zero entry; cost [nbin] is fully written. Scratch,
// contents unspecified on entry and exit: PE [Nbase, D, 2, 4], PG
// [Nbase, G, 2, 4], PC [Nbase, E]. hipErrorInvalidValue: a dimension < 1,
// 2 M > JOINT_JTJ_TB, or the time tile of M clusters beyond 64 KB of LDS
// (M > 30).
hipError_t launch_joint_jtj(JointJtjArgs a, float2* PE, float2* PG, float* PC,
                            float* H, float* g, float* cost,
                            hipStream_t stream);
// cost [nbin] alone, at the J of a; etab, gtab, sdst, gdst, cpos, sta_off
// and sta_ent are not read, and there is no H to touch.
hipError_t launch_joint_cost(JointJtjArgs a, float* PC, float* cost,
                             hipStream_t stream);

// Threads per workgroup of k_lbfgs_mf_res and pairs per tile of
// k_lbfgs_mf_grad.
#define LBFGS_MF_TB 256
// cost [1] and grad [Mt*N*8] float32, in the order of view_as_real(J), both
// fully written. Scratch, contents unspecified on entry and exit: sres
// [F, R, 4], slots [E, Nbase, 8], cpart [F * ceil(R / LBFGS_MF_TB)].
// hipErrorInvalidValue: a dimension < 1, F > 65535, Nbase / LBFGS_MF_TB >
// 65535 or N*32 bytes beyond 64 KB of LDS.
hipError_t launch_lbfgs_mf(LbfgsMfArgs a, float2* sres, float2* slots,
                           float* cpart, float* cost, float* grad,
                           hipStream_t stream);

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

// The shapelet sources of all channels in one launch, ADDED into the `out`
// of the launcher above of the same shape (launch_predict_coh_mf with the
// same mean, launch_residual_mf), after it on the same stream and with the
// same ch, bm and res. Channels a thread carries per pass, without E-Jones
// and with:
#ifndef SHAPELET_MF_NF
#define SHAPELET_MF_NF 2
#endif
#ifndef SHAPELET_MF_NF_EJ
#define SHAPELET_MF_NF_EJ 2
#endif
// hipErrorInvalidValue: what those two launchers refuse (res.x is not
// read: out holds x minus the model so far), S < 1, M < 1 or no entry_off.
hipError_t launch_shapelet_coh_mf(RowsUVW rows, ShapeletTabMF tab,
                                  Channels ch, BeamChannels bm, int mean,
                                  float2* out, hipStream_t stream);
hipError_t launch_shapelet_residual_mf(RowsUVW rows, ShapeletTabMF tab,
                                       Channels ch, BeamChannels bm,
                                       ResidualArgs res, float2* out,
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

// dp = (JtJ + mu I)^-1 Jtr, one workgroup per problem (chol_solve), the
// multi-workgroup kernel sequence (chol_mw) or the blocked sequence for
// n up to 16384 (chol_blocked); same contract, n a multiple of the block
// size, Lbuf 2*n*n floats per problem
hipError_t launch_chol_solve(
    const float* JtJ, const float* Jtr, const float* mu, int n, int batch,
    float* Lbuf, float* dp, int* info, hipStream_t stream);
hipError_t launch_chol_mw(
    const float* JtJ, const float* Jtr, const float* mu, int n, int batch,
    float* Lbuf, float* dp, int* info, hipStream_t stream);
hipError_t launch_chol_blocked(
    const float* JtJ, const float* Jtr, const float* mu, int n, int batch,
    float* Lbuf, float* dp, int* info, hipStream_t stream);

}  // extern "C"
