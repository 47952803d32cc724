// PyTorch bindings for the sagecal_amd gfx950 kernel library.
// Host-compiled: all kernel launches live in launchers.hip (hipcc).
#include <torch/extension.h>
#include <hip/hip_runtime.h>
#include <c10/hip/HIPStream.h>

#include "launchers.h"

#define CHECK_HIP(x) do { hipError_t e = (x); TORCH_CHECK(e == hipSuccess, \
    "HIP error: ", hipGetErrorString(e)); } while (0)

static hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

static float2* cptr(torch::Tensor& t) {
  return reinterpret_cast<float2*>(t.data_ptr());
}
static const float2* ccptr(const torch::Tensor& t) {
  return reinterpret_cast<const float2*>(t.data_ptr());
}
static const double* dp(const torch::Tensor& t) { return t.data_ptr<double>(); }
static const float* fp(const torch::Tensor& t) { return t.data_ptr<float>(); }
static const int* ip(const torch::Tensor& t) { return t.data_ptr<int>(); }
static RowsUVW rows_uvw(const torch::Tensor& u, const torch::Tensor& v,
                        const torch::Tensor& w) {
  RowsUVW rows = {};
  rows.u = dp(u); rows.v = dp(v); rows.w = dp(w);
  rows.R = (int)u.size(0);
  return rows;
}

// The optional station beam of both predict entry points: beam [T, K, N]
// float32, pairs [Nbase, 2] int32 and ejones [T, K, NE, 2, 2] complex64,
// checked against the rows of u. The kernels index all three by timeslot,
// source and station with no bounds of their own, and read pairs on every
// row with either buffer. Nsta_ej is the station count that ejones goes
// with (beam brings its own).
static BeamArgs beam_args(
    const c10::optional<torch::Tensor>& beam,
    const c10::optional<torch::Tensor>& pairs,
    const c10::optional<torch::Tensor>& ejones, const torch::Tensor& u,
    int64_t Nbase, int64_t Nsta_ej) {
  BeamArgs a = {};
  if (!beam.has_value() && !ejones.has_value()) return a;
  const int64_t R = u.size(0);
  TORCH_CHECK(pairs.has_value() && Nbase > 0,
              "beam and ejones need the station-pair table and Nbase");
  TORCH_CHECK(pairs->device() == u.device() &&
              pairs->scalar_type() == torch::kInt && pairs->is_contiguous() &&
              pairs->numel() == 2 * Nbase,
              "pairs must be contiguous [Nbase, 2] int32");
  a.pairs = pairs->data_ptr<int>();
  a.Nbase = (int)Nbase;
  if (beam.has_value()) {
    TORCH_CHECK(beam->device() == u.device() &&
                beam->scalar_type() == torch::kFloat &&
                beam->is_contiguous() && beam->dim() == 3,
                "beam must be contiguous [T, K, N] float32");
    TORCH_CHECK(R <= beam->size(0) * Nbase,
                "beam has too few timeslots for the rows");
    a.beam = beam->data_ptr<float>();
    a.Ktot = (int)beam->size(1);
    a.Nsta = (int)beam->size(2);
  }
  if (ejones.has_value()) {
    const torch::Tensor& e = *ejones;
    TORCH_CHECK(e.is_cuda() && e.device() == u.device() &&
                e.scalar_type() == torch::kComplexFloat &&
                e.is_contiguous() && e.dim() == 5 && e.size(3) == 2 &&
                e.size(4) == 2,
                "ejones must be contiguous [T, K, NE, 2, 2] complex64");
    TORCH_CHECK(e.size(0) * Nbase == R, "ejones timeslots * Nbase != rows");
    TORCH_CHECK(Nsta_ej > 0, "ejones needs the station count Nsta");
    TORCH_CHECK(e.size(2) == 1 || e.size(2) == Nsta_ej,
                "ejones must hold 1 or Nsta patterns per source");
    if (beam.has_value())
      TORCH_CHECK(beam->size(0) == e.size(0) && beam->size(1) == e.size(1) &&
                  beam->size(2) == Nsta_ej,
                  "beam and ejones disagree on [T, K] or Nsta");
    a.ejones = ccptr(e);
    a.NE = (int)e.size(2);
    a.Ktot = (int)e.size(1);
    a.Nsta = (int)Nsta_ej;
  }
  return a;
}

torch::Tensor predict_coh(
    torch::Tensor u, torch::Tensor v, torch::Tensor w,
    torch::Tensor ll, torch::Tensor mm, torch::Tensor nn1,
    torch::Tensor sI, torch::Tensor sQ, torch::Tensor sU, torch::Tensor sV,
    torch::Tensor eX, torch::Tensor eY, torch::Tensor eP,
    torch::Tensor cxi, torch::Tensor sxi, torch::Tensor cphi,
    torch::Tensor sphi, torch::Tensor r1, torch::Tensor stype,
    torch::Tensor cluster_off, double freq, double fdelta2, double tdelta,
    c10::optional<torch::Tensor> beam, c10::optional<torch::Tensor> pairs,
    int64_t Nbase, c10::optional<torch::Tensor> ejones, int64_t Nsta_ej) {
  const BeamArgs bm = beam_args(beam, pairs, ejones, u, Nbase, Nsta_ej);
  const RowsUVW rows = rows_uvw(u, v, w);
  SourceArrays src = {};
  src.ll = dp(ll); src.mm = dp(mm); src.nn1 = dp(nn1);
  src.sI = fp(sI); src.sQ = fp(sQ); src.sU = fp(sU); src.sV = fp(sV);
  src.eX = fp(eX); src.eY = fp(eY); src.eP = fp(eP);
  src.cxi = fp(cxi); src.sxi = fp(sxi); src.cphi = fp(cphi);
  src.sphi = fp(sphi); src.r1 = fp(r1);
  src.stype = ip(stype); src.cluster_off = ip(cluster_off);
  src.M = (int)cluster_off.size(0) - 1;
  auto out = torch::empty({src.M, rows.R, 4},
      torch::dtype(torch::kComplexFloat).device(u.device()));
  CHECK_HIP(launch_predict_coh(rows, src, {freq, fdelta2, tdelta}, bm,
                               cptr(out), cur_stream()));
  return out;
}

// Adds the shapelet sources of a ShapeletTable (hip_host.py) into `out`
// [M, R, 4] complex64, in place, on the current stream.
void shapelet_coh_add(
    torch::Tensor out, torch::Tensor u, torch::Tensor v, torch::Tensor w,
    torch::Tensor src, torch::Tensor cluster, torch::Tensor n0,
    torch::Tensor beta, torch::Tensor off, torch::Tensor coef,
    torch::Tensor cxi, torch::Tensor sxi, torch::Tensor cphi,
    torch::Tensor sphi, torch::Tensor psign, torch::Tensor a,
    torch::Tensor b, torch::Tensor ceP, torch::Tensor seP,
    torch::Tensor ll, torch::Tensor mm, torch::Tensor nn1,
    torch::Tensor rec, torch::Tensor flux, torch::Tensor r1,
    double freq, double fdelta2, double tdelta,
    c10::optional<torch::Tensor> beam, c10::optional<torch::Tensor> pairs,
    int64_t Nbase, c10::optional<torch::Tensor> ejones, int64_t Nsta_ej) {
  const int64_t R = u.size(0);
  const int64_t S = src.size(0);
  auto chk = [&](const torch::Tensor& t, torch::ScalarType ty, int64_t n,
                 const char* name) {
    TORCH_CHECK(t.device() == out.device(), name, " is on another device");
    TORCH_CHECK(t.scalar_type() == ty, name, " has the wrong dtype");
    TORCH_CHECK(t.is_contiguous() && t.numel() == n, name,
                " must be contiguous with ", n, " elements");
  };
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kComplexFloat &&
              out.is_contiguous() && out.dim() == 3 && out.size(1) == R &&
              out.size(2) == 4, "out must be contiguous [M, R, 4] complex64");
  chk(u, torch::kDouble, R, "u");
  chk(v, torch::kDouble, R, "v");
  chk(w, torch::kDouble, R, "w");
  chk(src, torch::kInt, S, "src");
  chk(cluster, torch::kInt, S, "cluster");
  chk(n0, torch::kInt, S, "n0");
  chk(beta, torch::kFloat, S, "beta");
  chk(off, torch::kInt, S + 1, "off");
  TORCH_CHECK(coef.scalar_type() == torch::kFloat && coef.is_contiguous() &&
              coef.device() == out.device(), "coef must be contiguous float32");
  chk(cxi, torch::kFloat, S, "cxi");
  chk(sxi, torch::kFloat, S, "sxi");
  chk(cphi, torch::kFloat, S, "cphi");
  chk(sphi, torch::kFloat, S, "sphi");
  chk(psign, torch::kFloat, S, "psign");
  chk(a, torch::kFloat, S, "a");
  chk(b, torch::kFloat, S, "b");
  chk(ceP, torch::kFloat, S, "ceP");
  chk(seP, torch::kFloat, S, "seP");
  chk(ll, torch::kDouble, S, "ll");
  chk(mm, torch::kDouble, S, "mm");
  chk(nn1, torch::kDouble, S, "nn1");
  TORCH_CHECK(rec.dim() == 2 && rec.size(0) == 2, "rec must be [2, max n0]");
  chk(rec, torch::kFloat, rec.numel(), "rec");
  chk(flux, torch::kFloat, 4 * S, "flux");
  chk(r1, torch::kFloat, S, "r1");
  const BeamArgs bm = beam_args(beam, pairs, ejones, u, Nbase, Nsta_ej);
  ShapeletTab tab = {};
  tab.src = ip(src); tab.cluster = ip(cluster); tab.n0 = ip(n0);
  tab.beta = fp(beta); tab.off = ip(off); tab.coef = fp(coef);
  tab.cxi = fp(cxi); tab.sxi = fp(sxi); tab.cphi = fp(cphi);
  tab.sphi = fp(sphi); tab.psign = fp(psign); tab.a = fp(a); tab.b = fp(b);
  tab.ceP = fp(ceP); tab.seP = fp(seP);
  tab.ll = dp(ll); tab.mm = dp(mm); tab.nn1 = dp(nn1);
  tab.rec = fp(rec); tab.S = (int)S; tab.nmax = (int)rec.size(1);
  tab.flux = fp(flux); tab.r1 = fp(r1);
  CHECK_HIP(launch_shapelet_coh(rows_uvw(u, v, w), tab,
                                {freq, fdelta2, tdelta}, bm, cptr(out),
                                cur_stream()));
}

// The arguments the two all-channels entry points share, checked: every
// per-source tensor has K entries, flux is [F, 4, K] float32 (I, Q, U, V
// rows per channel), freqs [F] float64, all on u's device and contiguous.
struct MfArgs {
  RowsUVW rows;
  SourceArrays src;
  Channels ch;
};

static MfArgs mf_args(
    const torch::Tensor& u, const torch::Tensor& v, const torch::Tensor& w,
    const torch::Tensor& ll, const torch::Tensor& mm,
    const torch::Tensor& nn1, const torch::Tensor& flux,
    const torch::Tensor& eX, const torch::Tensor& eY,
    const torch::Tensor& eP, const torch::Tensor& cxi,
    const torch::Tensor& sxi, const torch::Tensor& cphi,
    const torch::Tensor& sphi, const torch::Tensor& r1,
    const torch::Tensor& stype, const torch::Tensor& cluster_off,
    const torch::Tensor& freqs, double fdelta2, double tdelta) {
  TORCH_CHECK(u.is_cuda() && u.dim() == 1, "u must be a device tensor [R]");
  const int64_t R = u.size(0), K = ll.size(0);
  auto chk = [&](const torch::Tensor& t, torch::ScalarType ty, int64_t n,
                 const char* name) {
    TORCH_CHECK(t.device() == u.device(), name, " is on another device");
    TORCH_CHECK(t.scalar_type() == ty, name, " has the wrong dtype");
    TORCH_CHECK(t.is_contiguous() && t.numel() == n, name,
                " must be contiguous with ", n, " elements");
  };
  chk(u, torch::kDouble, R, "u");
  chk(v, torch::kDouble, R, "v");
  chk(w, torch::kDouble, R, "w");
  chk(ll, torch::kDouble, K, "ll");
  chk(mm, torch::kDouble, K, "mm");
  chk(nn1, torch::kDouble, K, "nn1");
  chk(eX, torch::kFloat, K, "eX");
  chk(eY, torch::kFloat, K, "eY");
  chk(eP, torch::kFloat, K, "eP");
  chk(cxi, torch::kFloat, K, "cxi");
  chk(sxi, torch::kFloat, K, "sxi");
  chk(cphi, torch::kFloat, K, "cphi");
  chk(sphi, torch::kFloat, K, "sphi");
  chk(r1, torch::kFloat, K, "r1");
  chk(stype, torch::kInt, K, "stype");
  TORCH_CHECK(freqs.dim() == 1 && freqs.size(0) >= 1, "freqs must be [F], "
              "F >= 1");
  const int64_t F = freqs.size(0);
  chk(freqs, torch::kDouble, F, "freqs");
  TORCH_CHECK(flux.dim() == 3 && flux.size(0) == F && flux.size(1) == 4,
              "flux must be [F, 4, K]");
  chk(flux, torch::kFloat, F * 4 * K, "flux");
  TORCH_CHECK(cluster_off.dim() == 1 && cluster_off.size(0) >= 1,
              "cluster_off must be [M + 1]");
  chk(cluster_off, torch::kInt, cluster_off.size(0), "cluster_off");
  TORCH_CHECK(R >= 1 && R < (int64_t(1) << 31), "rows out of range");
  MfArgs a = {};
  a.rows = rows_uvw(u, v, w);
  a.src.ll = dp(ll); a.src.mm = dp(mm); a.src.nn1 = dp(nn1);
  a.src.sI = fp(flux); a.src.sQ = fp(flux) + K;
  a.src.sU = fp(flux) + 2 * K; a.src.sV = fp(flux) + 3 * K;
  a.src.eX = fp(eX); a.src.eY = fp(eY); a.src.eP = fp(eP);
  a.src.cxi = fp(cxi); a.src.sxi = fp(sxi); a.src.cphi = fp(cphi);
  a.src.sphi = fp(sphi); a.src.r1 = fp(r1);
  a.src.stype = ip(stype); a.src.cluster_off = ip(cluster_off);
  a.src.M = (int)cluster_off.size(0) - 1;
  a.ch.freqs = dp(freqs);
  a.ch.F = (int)F;
  a.ch.fdelta2 = fdelta2;
  a.ch.tdelta = tdelta;
  a.ch.flux_stride = 4 * K;
  return a;
}

// The optional station beam of the two all-channels entry points: beam
// [F, T, Ke, N] float32, ejones [F, T, Ke, NE, 2, 2] complex64 and pairs
// [Nbase, 2] int32, checked against the F channels, R rows and K sources of
// `a`. The kernels index the buffers by channel, timeslot, source and
// station with no bounds of their own; the caller guarantees pair entries
// below the station count (negative ones only where the kernel keeps x).
// Nsta_ej is the station count that ejones goes with (beam brings its own).
static BeamChannels beam_channels(
    const c10::optional<torch::Tensor>& beam,
    const c10::optional<torch::Tensor>& ejones,
    const c10::optional<torch::Tensor>& pairs, int64_t Nbase,
    int64_t Nsta_ej, const MfArgs& a, int64_t K, const torch::Tensor& u) {
  BeamChannels b = {};
  if (!beam.has_value() && !ejones.has_value()) return b;
  const int64_t R = a.rows.R, F = a.ch.F;
  TORCH_CHECK(pairs.has_value() && Nbase > 0,
              "beam and ejones need the station-pair table and Nbase");
  TORCH_CHECK(pairs->device() == u.device() &&
              pairs->scalar_type() == torch::kInt && pairs->is_contiguous() &&
              pairs->numel() == 2 * Nbase,
              "pairs must be contiguous [Nbase, 2] int32");
  TORCH_CHECK(R % Nbase == 0, "rows must be T * Nbase");
  const int64_t T = R / Nbase;
  b.pairs = pairs->data_ptr<int>();
  b.Nbase = (int)Nbase;
  b.T = (int)T;
  auto fits = [](int64_t n) { return n >= 1 && n < (int64_t(1) << 31); };
  if (beam.has_value()) {
    const torch::Tensor& g = *beam;
    TORCH_CHECK(g.device() == u.device() &&
                g.scalar_type() == torch::kFloat && g.is_contiguous() &&
                g.dim() == 4, "beam must be contiguous [F, T, K, N] float32");
    TORCH_CHECK(g.size(0) == F && g.size(1) == T,
                "beam must hold the F channels and T timeslots of the rows");
    TORCH_CHECK(g.size(2) >= K && fits(g.size(2)) && fits(g.size(3)),
                "beam covers fewer sources than the pack");
    b.beam = g.data_ptr<float>();
    b.Ktot = (int)g.size(2);
    b.Nsta = (int)g.size(3);
  }
  if (ejones.has_value()) {
    const torch::Tensor& e = *ejones;
    TORCH_CHECK(e.device() == u.device() &&
                e.scalar_type() == torch::kComplexFloat &&
                e.is_contiguous() && e.dim() == 6 && e.size(4) == 2 &&
                e.size(5) == 2,
                "ejones must be contiguous [F, T, K, NE, 2, 2] complex64");
    TORCH_CHECK(e.size(0) == F && e.size(1) == T,
                "ejones must hold the F channels and T timeslots of the rows");
    TORCH_CHECK(e.size(2) >= K && fits(e.size(2)),
                "ejones covers fewer sources than the pack");
    TORCH_CHECK(fits(Nsta_ej), "ejones needs the station count Nsta");
    TORCH_CHECK(e.size(3) == 1 || e.size(3) == Nsta_ej,
                "ejones must hold 1 or Nsta patterns per source");
    if (beam.has_value())
      TORCH_CHECK(beam->size(2) == e.size(2) && beam->size(3) == Nsta_ej,
                  "beam and ejones disagree on K or Nsta");
    b.ejones = ccptr(e);
    b.NE = (int)e.size(3);
    b.Ktot = (int)e.size(2);
    b.Nsta = (int)Nsta_ej;
  }
  return b;
}

// Coherencies of all F channels in one launch (k_predict_coh_mf):
// [F, M, R, 4] complex64, or with mean their channel mean [M, R, 4]
// (k_predict_coh_mean); with beam and/or ejones the _bm / _ej kernels. The
// caller guarantees that cluster_off is non-decreasing from 0 to K.
torch::Tensor predict_coh_channels(
    torch::Tensor u, torch::Tensor v, torch::Tensor w,
    torch::Tensor ll, torch::Tensor mm, torch::Tensor nn1,
    torch::Tensor flux, torch::Tensor eX, torch::Tensor eY, torch::Tensor eP,
    torch::Tensor cxi, torch::Tensor sxi, torch::Tensor cphi,
    torch::Tensor sphi, torch::Tensor r1, torch::Tensor stype,
    torch::Tensor cluster_off, torch::Tensor freqs, double fdelta2,
    double tdelta, bool mean, c10::optional<torch::Tensor> beam,
    c10::optional<torch::Tensor> ejones, c10::optional<torch::Tensor> pairs,
    int64_t Nbase, int64_t Nsta_ej) {
  const MfArgs a = mf_args(u, v, w, ll, mm, nn1, flux, eX, eY, eP, cxi, sxi,
                           cphi, sphi, r1, stype, cluster_off, freqs,
                           fdelta2, tdelta);
  const BeamChannels bm = beam_channels(beam, ejones, pairs, Nbase, Nsta_ej,
                                        a, ll.size(0), u);
  auto copts = torch::dtype(torch::kComplexFloat).device(u.device());
  auto out = mean ? torch::empty({a.src.M, a.rows.R, 4}, copts)
                  : torch::empty({a.ch.F, a.src.M, a.rows.R, 4}, copts);
  CHECK_HIP(launch_predict_coh_mf(a.rows, a.src, a.ch, bm, mean ? 1 : 0,
                                  cptr(out), cur_stream()));
  return out;
}

// x - sum over clusters with skip == 0 of J_p C J_q^H for all F channels in
// one launch (k_residual_mf): x [F, R, 4] complex64, J [Mt, N, 4]
// complex64, chunk_tab [M, T] int32 global chunk ids, pairs [Nbase, 2]
// int32, R == T * Nbase, skip [M] int32 or none. Returns [F, R, 4]. The
// caller guarantees chunk ids below Mt and pair entries below N. With beam
// [F, T, Ke, Nsta] and/or ejones [F, T, Ke, NE, 2, 2] the coherencies carry
// the station beam (k_residual_mf_bm / _ej), indexed through the same pairs.
torch::Tensor residuals_multifreq(
    torch::Tensor x, torch::Tensor u, torch::Tensor v, torch::Tensor w,
    torch::Tensor ll, torch::Tensor mm, torch::Tensor nn1,
    torch::Tensor flux, torch::Tensor eX, torch::Tensor eY, torch::Tensor eP,
    torch::Tensor cxi, torch::Tensor sxi, torch::Tensor cphi,
    torch::Tensor sphi, torch::Tensor r1, torch::Tensor stype,
    torch::Tensor cluster_off, torch::Tensor freqs, double fdelta2,
    double tdelta, torch::Tensor J, torch::Tensor chunk_tab,
    torch::Tensor pairs, c10::optional<torch::Tensor> skip,
    c10::optional<torch::Tensor> beam, c10::optional<torch::Tensor> ejones,
    int64_t Nsta_ej) {
  const MfArgs a = mf_args(u, v, w, ll, mm, nn1, flux, eX, eY, eP, cxi, sxi,
                           cphi, sphi, r1, stype, cluster_off, freqs,
                           fdelta2, tdelta);
  const int64_t R = a.rows.R, F = a.ch.F, M = a.src.M;
  auto on_dev = [&](const torch::Tensor& t, torch::ScalarType ty) {
    return t.device() == u.device() && t.scalar_type() == ty &&
           t.is_contiguous();
  };
  TORCH_CHECK(on_dev(x, torch::kComplexFloat) && x.dim() == 3 &&
              x.size(0) == F && x.size(1) == R && x.size(2) == 4,
              "x must be contiguous [F, R, 4] complex64");
  TORCH_CHECK(on_dev(J, torch::kComplexFloat) && J.dim() == 3 &&
              J.size(0) >= 1 && J.size(1) >= 1 && J.size(2) == 4,
              "J must be contiguous [Mt, N, 4] complex64");
  TORCH_CHECK(on_dev(chunk_tab, torch::kInt) && chunk_tab.dim() == 2 &&
              chunk_tab.size(0) == M && chunk_tab.size(1) >= 1,
              "chunk_tab must be contiguous [M, T] int32");
  TORCH_CHECK(on_dev(pairs, torch::kInt) && pairs.dim() == 2 &&
              pairs.size(0) >= 1 && pairs.size(1) == 2,
              "pairs must be contiguous [Nbase, 2] int32");
  TORCH_CHECK(chunk_tab.size(1) * pairs.size(0) == R,
              "rows must be T * Nbase");
  ResidualArgs res = {};
  res.x = ccptr(x);
  res.J = ccptr(J);
  res.chunk_tab = ip(chunk_tab);
  res.pairs = ip(pairs);
  if (skip.has_value()) {
    TORCH_CHECK(on_dev(*skip, torch::kInt) && skip->numel() == M,
                "skip must be contiguous [M] int32");
    res.skip = ip(*skip);
  }
  res.Nbase = (int)pairs.size(0);
  res.T = (int)chunk_tab.size(1);
  res.N = (int)J.size(1);
  const BeamChannels bm = beam_channels(beam, ejones, pairs, pairs.size(0),
                                        Nsta_ej, a, ll.size(0), u);
  auto out = torch::empty({F, R, 4},
      torch::dtype(torch::kComplexFloat).device(u.device()));
  CHECK_HIP(launch_residual_mf(a.rows, a.src, a.ch, bm, res, cptr(out),
                               cur_stream()));
  return out;
}

// The four tensors both beam-gain entry points share: elem [N, Emax, 3]
// float64 on the device, nelem [N] int32 (the caller has checked
// 1 <= nelem <= Emax on the host), du [T, K, 3] float64, below [T, K] uint8.
static void check_beam_geometry(
    const torch::Tensor& elem, const torch::Tensor& nelem,
    const torch::Tensor& du, const torch::Tensor& below) {
  TORCH_CHECK(elem.is_cuda() && elem.scalar_type() == torch::kDouble &&
              elem.is_contiguous() && elem.dim() == 3 && elem.size(2) == 3 &&
              elem.size(1) > 0, "elem must be contiguous [N, Emax, 3] float64");
  TORCH_CHECK(nelem.device() == elem.device() &&
              nelem.scalar_type() == torch::kInt && nelem.is_contiguous() &&
              nelem.numel() == elem.size(0),
              "nelem must be contiguous [N] int32");
  TORCH_CHECK(du.device() == elem.device() &&
              du.scalar_type() == torch::kDouble && du.is_contiguous() &&
              du.dim() == 3 && du.size(2) == 3,
              "du must be contiguous [T, K, 3] float64");
  TORCH_CHECK(below.device() == elem.device() &&
              below.scalar_type() == torch::kByte && below.is_contiguous() &&
              below.dim() == 2 && below.size(0) == du.size(0) &&
              below.size(1) == du.size(1),
              "below must be contiguous [T, K] uint8");
  TORCH_CHECK(du.size(0) * du.size(1) < (int64_t(1) << 31),
              "too many (timeslot, source) pairs");
}

// gain[t,k,n] of k_array_beam for the tensors of check_beam_geometry and
// kf = 2 pi f / c. Returns [T, K, N] float32.
torch::Tensor array_beam_gains(
    torch::Tensor elem, torch::Tensor nelem, torch::Tensor du,
    torch::Tensor below, double kf) {
  check_beam_geometry(elem, nelem, du, below);
  const int64_t N = elem.size(0), Emax = elem.size(1);
  const int64_t T = du.size(0), K = du.size(1);
  auto gain = torch::empty({T, K, N},
      torch::dtype(torch::kFloat).device(elem.device()));
  CHECK_HIP(launch_array_beam(elem.data_ptr<double>(), nelem.data_ptr<int>(),
      du.data_ptr<double>(), below.data_ptr<uint8_t>(), (int)N, (int)Emax,
      (int)(T * K), kf, gain.data_ptr<float>(), cur_stream()));
  return gain;
}

// gain[f,t,k,n] of k_station_beam. elem, nelem, du and below as for
// array_beam_gains; kf [F] float64 wavenumbers 2 pi f / c; tile [N, D, 3]
// float64 dipole offsets inside a tile and du_tile [T, K, 3] float64, given
// together (two-stage) or not at all (single stage), 1 <= D <= 64.
// Returns [F, T, K, N] float32.
torch::Tensor station_beam_gains(
    torch::Tensor elem, torch::Tensor nelem, torch::Tensor du,
    torch::Tensor below, torch::Tensor kf,
    c10::optional<torch::Tensor> tile, c10::optional<torch::Tensor> du_tile) {
  check_beam_geometry(elem, nelem, du, below);
  const int64_t N = elem.size(0), Emax = elem.size(1);
  const int64_t T = du.size(0), K = du.size(1);
  TORCH_CHECK(kf.device() == elem.device() &&
              kf.scalar_type() == torch::kDouble && kf.is_contiguous() &&
              kf.dim() == 1, "kf must be contiguous [F] float64");
  const int64_t F = kf.size(0);
  TORCH_CHECK(tile.has_value() == du_tile.has_value(),
              "tile and du_tile come together");
  const double* tile_p = nullptr;
  const double* dut_p = nullptr;
  int64_t D = 0;
  if (tile.has_value()) {
    const torch::Tensor& tl = *tile;
    const torch::Tensor& dt = *du_tile;
    TORCH_CHECK(tl.device() == elem.device() &&
                tl.scalar_type() == torch::kDouble && tl.is_contiguous() &&
                tl.dim() == 3 && tl.size(0) == N && tl.size(2) == 3 &&
                tl.size(1) >= 1 && tl.size(1) <= 64,
                "tile must be contiguous [N, D, 3] float64, 1 <= D <= 64");
    TORCH_CHECK(dt.device() == elem.device() &&
                dt.scalar_type() == torch::kDouble && dt.is_contiguous() &&
                dt.dim() == 3 && dt.size(0) == T && dt.size(1) == K &&
                dt.size(2) == 3,
                "du_tile must be contiguous [T, K, 3] float64");
    D = tl.size(1);
    tile_p = tl.data_ptr<double>();
    dut_p = dt.data_ptr<double>();
  }
  auto gain = torch::empty({F, T, K, N},
      torch::dtype(torch::kFloat).device(elem.device()));
  CHECK_HIP(launch_station_beam(elem.data_ptr<double>(),
      nelem.data_ptr<int>(), tile_p, du.data_ptr<double>(), dut_p,
      below.data_ptr<uint8_t>(), kf.data_ptr<double>(), (int)N, (int)Emax,
      (int)D, (int)(T * K), (int)F, gain.data_ptr<float>(), cur_stream()));
  return gain;
}

// E[f,d] of k_element_beam: az, el [D] float64 directions, coef
// [F, 2, Nmodes] complex64 theta and phi coefficient rows per frequency,
// preamble [Nmodes] float32, Nmodes = M(M+1)/2 with 1 <= M <=
// ELEMENT_BEAM_MAX_M, beta > 0. Returns [F, D, 2, 2] complex64.
torch::Tensor element_jones(
    torch::Tensor az, torch::Tensor el, torch::Tensor coef,
    torch::Tensor preamble, int64_t M, double beta) {
  TORCH_CHECK(M >= 1 && M <= ELEMENT_BEAM_MAX_M, "M must be 1..",
              ELEMENT_BEAM_MAX_M, ", got ", M);
  TORCH_CHECK(beta > 0.0 && (float)beta > 0.f, "beta must be positive");
  const int64_t Nmodes = M * (M + 1) / 2;
  TORCH_CHECK(az.is_cuda() && az.scalar_type() == torch::kDouble &&
              az.is_contiguous() && az.dim() == 1,
              "az must be contiguous [D] float64 on the device");
  TORCH_CHECK(el.device() == az.device() &&
              el.scalar_type() == torch::kDouble && el.is_contiguous() &&
              el.dim() == 1 && el.size(0) == az.size(0),
              "el must be contiguous [D] float64 like az");
  TORCH_CHECK(coef.device() == az.device() &&
              coef.scalar_type() == torch::kComplexFloat &&
              coef.is_contiguous() && coef.dim() == 3 && coef.size(0) >= 1 &&
              coef.size(1) == 2 && coef.size(2) == Nmodes,
              "coef must be contiguous [F, 2, M(M+1)/2] complex64, F >= 1");
  TORCH_CHECK(preamble.device() == az.device() &&
              preamble.scalar_type() == torch::kFloat &&
              preamble.is_contiguous() && preamble.dim() == 1 &&
              preamble.size(0) == Nmodes,
              "preamble must be contiguous [M(M+1)/2] float32");
  const int64_t D = az.size(0), F = coef.size(0);
  TORCH_CHECK(D < (int64_t(1) << 31) && F < (int64_t(1) << 31),
              "too many directions or frequencies");
  auto E = torch::empty({F, D, 2, 2},
      torch::dtype(torch::kComplexFloat).device(az.device()));
  CHECK_HIP(launch_element_beam(az.data_ptr<double>(), el.data_ptr<double>(),
      ccptr(coef), preamble.data_ptr<float>(), (int)D, (int)F, (int)M,
      (float)beta, cptr(E), cur_stream()));
  return E;
}

std::vector<torch::Tensor> jtj_jtr(
    torch::Tensor x, torch::Tensor coh, torch::Tensor J,
    torch::Tensor pairs, torch::Tensor chunk_tab, torch::Tensor pidx,
    c10::optional<torch::Tensor> wts, int64_t Nbase, int64_t T, int64_t N,
    int64_t nseg, int64_t Mt) {
  auto fopts = torch::dtype(torch::kFloat).device(x.device());
  auto copts = torch::dtype(torch::kComplexFloat).device(x.device());
  const int64_t npair = Nbase;
  auto D = torch::zeros({Mt * N, 4}, copts);
  auto g = torch::zeros({Mt * N, 4}, copts);
  auto Cx = torch::zeros({Mt * npair, 16}, copts);
  auto cost = torch::zeros({Mt}, fopts);
  // per-(chunk, pair) partial slots of the store pass; only slots of
  // chunks marked present are read back
  auto PD = torch::empty({Mt * npair, 8}, copts);
  auto Pg = torch::empty({Mt * npair, 8}, copts);
  auto Pc = torch::empty({Mt * npair}, fopts);
  auto present = torch::zeros({Mt},
      torch::dtype(torch::kInt).device(x.device()));
  const float* wp = wts.has_value() ? wts->data_ptr<float>() : nullptr;
  CHECK_HIP(launch_jtj_accum(ccptr(x), ccptr(coh), ccptr(J),
      pairs.data_ptr<int>(), chunk_tab.data_ptr<int>(),
      pidx.data_ptr<int>(), wp, (int)Nbase, (int)T, (int)N, (int)nseg,
      (int)Mt, cptr(PD), cptr(Pg), Pc.data_ptr<float>(),
      present.data_ptr<int>(), cptr(D), cptr(g), cptr(Cx),
      cost.data_ptr<float>(), (int)npair, 0, cur_stream()));
  auto JtJ = torch::empty({Mt, 8 * N, 8 * N}, fopts);
  auto Jtr = torch::empty({Mt, 8 * N}, fopts);
  CHECK_HIP(launch_jtj_expand(ccptr(D), ccptr(g), ccptr(Cx),
      pairs.data_ptr<int>(), pidx.data_ptr<int>(), (int)N, (int)npair,
      (int)Mt,
      JtJ.data_ptr<float>(), Jtr.data_ptr<float>(), cur_stream()));
  return {JtJ, Jtr, cost};
}

torch::Tensor model_cost(
    torch::Tensor x, torch::Tensor coh, torch::Tensor J,
    torch::Tensor pairs, torch::Tensor chunk_tab,
    c10::optional<torch::Tensor> wts, int64_t Nbase, int64_t T, int64_t N,
    int64_t nseg, int64_t Mt) {
  auto fopts = torch::dtype(torch::kFloat).device(x.device());
  auto cost = torch::zeros({Mt}, fopts);
  // per-row cost, then one sum per (seg, t) slot
  auto e2 = torch::empty({nseg * T * Nbase + nseg * T}, fopts);
  const float* wp = wts.has_value() ? wts->data_ptr<float>() : nullptr;
  CHECK_HIP(launch_model_cost(ccptr(x), ccptr(coh), ccptr(J),
      pairs.data_ptr<int>(), chunk_tab.data_ptr<int>(), wp,
      (int)Nbase, (int)T, (int)N, (int)nseg, (int)Mt,
      e2.data_ptr<float>(), cost.data_ptr<float>(), cur_stream()));
  return cost;
}

torch::Tensor apply_jones(
    c10::optional<torch::Tensor> x, torch::Tensor cohs, torch::Tensor J,
    torch::Tensor pairs, torch::Tensor chunk_tab, int64_t Nbase, int64_t T,
    int64_t N, int64_t nseg, int64_t M, int64_t sub) {
  const int64_t B = nseg * T * Nbase;
  auto out = torch::empty({B, 4},
      torch::dtype(torch::kComplexFloat).device(cohs.device()));
  const float2* xp = x.has_value() ? ccptr(*x) : nullptr;
  CHECK_HIP(launch_apply_jones(xp, ccptr(cohs), ccptr(J),
      pairs.data_ptr<int>(), chunk_tab.data_ptr<int>(), (int)Nbase, (int)T,
      (int)N, (int)nseg, (int)M, (int)sub, cptr(out), cur_stream()));
  return out;
}

using chol_launcher_t = hipError_t (*)(const float*, const float*,
    const float*, int, int, float*, float*, int*, hipStream_t);

// dp = (JtJ + mu I)^-1 Jtr through either Cholesky launcher (same
// contract); scratch holds 2*n*n floats per problem
static std::vector<torch::Tensor> chol_solve_with(
    chol_launcher_t launch, torch::Tensor JtJ, torch::Tensor Jtr,
    torch::Tensor mu, torch::Tensor scratch) {
  TORCH_CHECK(JtJ.dim() == 3 && JtJ.size(1) == JtJ.size(2),
              "JtJ must be [batch, n, n]");
  const int64_t batch = JtJ.size(0);
  const int64_t n = JtJ.size(1);
  TORCH_CHECK(Jtr.dim() == 2 && Jtr.size(0) == batch && Jtr.size(1) == n,
              "Jtr must be [batch, n]");
  TORCH_CHECK(mu.dim() == 1 && mu.size(0) == batch, "mu must be [batch]");
  TORCH_CHECK(JtJ.is_contiguous() && Jtr.is_contiguous() &&
              mu.is_contiguous() && scratch.is_contiguous(),
              "JtJ, Jtr, mu and scratch must be contiguous");
  TORCH_CHECK(scratch.numel() >= batch * 2 * n * n,
              "scratch must hold batch * 2 * n * n floats");
  auto dp = torch::empty({batch, n},
      torch::dtype(torch::kFloat).device(JtJ.device()));
  auto info = torch::zeros({batch},
      torch::dtype(torch::kInt).device(JtJ.device()));
  CHECK_HIP(launch(JtJ.data_ptr<float>(), Jtr.data_ptr<float>(),
      mu.data_ptr<float>(), (int)n, (int)batch, scratch.data_ptr<float>(),
      dp.data_ptr<float>(), info.data_ptr<int>(), cur_stream()));
  return {dp, info};
}

std::vector<torch::Tensor> chol_solve(
    torch::Tensor JtJ, torch::Tensor Jtr, torch::Tensor mu,
    torch::Tensor scratch) {
  return chol_solve_with(launch_chol_solve, JtJ, Jtr, mu, scratch);
}

std::vector<torch::Tensor> chol_solve_mw(
    torch::Tensor JtJ, torch::Tensor Jtr, torch::Tensor mu,
    torch::Tensor scratch) {
  return chol_solve_with(launch_chol_mw, JtJ, Jtr, mu, scratch);
}

std::vector<torch::Tensor> jtr_grad(
    torch::Tensor x, torch::Tensor coh, torch::Tensor J,
    torch::Tensor pairs, torch::Tensor chunk_tab, torch::Tensor pidx,
    c10::optional<torch::Tensor> wts, int64_t Nbase, int64_t T, int64_t N,
    int64_t nseg, int64_t Mt) {
  // gradient-only accumulation (LBFGS path): returns (g [Mt*N,4] c64,
  // cost [Mt]); g's interleaved memory IS vecR order.
  auto fopts = torch::dtype(torch::kFloat).device(x.device());
  auto copts = torch::dtype(torch::kComplexFloat).device(x.device());
  auto g = torch::zeros({Mt * N, 4}, copts);
  auto cost = torch::zeros({Mt}, fopts);
  auto Pg = torch::empty({Mt * Nbase, 8}, copts);
  auto Pc = torch::empty({Mt * Nbase}, fopts);
  auto present = torch::zeros({Mt},
      torch::dtype(torch::kInt).device(x.device()));
  const float* wp = wts.has_value() ? wts->data_ptr<float>() : nullptr;
  CHECK_HIP(launch_jtj_accum(ccptr(x), ccptr(coh), ccptr(J),
      pairs.data_ptr<int>(), chunk_tab.data_ptr<int>(),
      pidx.data_ptr<int>(), wp, (int)Nbase, (int)T, (int)N, (int)nseg,
      (int)Mt, nullptr, cptr(Pg), Pc.data_ptr<float>(),
      present.data_ptr<int>(), nullptr, cptr(g), nullptr,
      cost.data_ptr<float>(), (int)Nbase, 1, cur_stream()));
  return {g, cost};
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("jtr_grad", &jtr_grad, "gradient-only accumulation (gfx950)");
  m.def("chol_solve", &chol_solve, "batched damped Cholesky solve (gfx950)");
  m.def("chol_solve_mw", &chol_solve_mw,
        "multi-workgroup damped Cholesky solve (gfx950)");
  m.def("predict_coh", &predict_coh, "coherency predict (gfx950)",
        py::arg("u"), py::arg("v"), py::arg("w"), py::arg("ll"),
        py::arg("mm"), py::arg("nn1"), py::arg("sI"), py::arg("sQ"),
        py::arg("sU"), py::arg("sV"), py::arg("eX"), py::arg("eY"),
        py::arg("eP"), py::arg("cxi"), py::arg("sxi"), py::arg("cphi"),
        py::arg("sphi"), py::arg("r1"), py::arg("stype"),
        py::arg("cluster_off"), py::arg("freq"), py::arg("fdelta2"),
        py::arg("tdelta"), py::arg("beam") = py::none(),
        py::arg("pairs") = py::none(), py::arg("Nbase") = 0,
        py::arg("ejones") = py::none(), py::arg("Nsta") = 0);
  m.def("shapelet_coh_add", &shapelet_coh_add,
        "add shapelet-source coherencies into out (gfx950)",
        py::arg("out"), py::arg("u"), py::arg("v"), py::arg("w"),
        py::arg("src"), py::arg("cluster"), py::arg("n0"), py::arg("beta"),
        py::arg("off"), py::arg("coef"), py::arg("cxi"), py::arg("sxi"),
        py::arg("cphi"), py::arg("sphi"), py::arg("psign"), py::arg("a"),
        py::arg("b"), py::arg("ceP"), py::arg("seP"), py::arg("ll"),
        py::arg("mm"), py::arg("nn1"), py::arg("rec"), py::arg("flux"),
        py::arg("r1"), py::arg("freq"), py::arg("fdelta2"),
        py::arg("tdelta"), py::arg("beam") = py::none(),
        py::arg("pairs") = py::none(), py::arg("Nbase") = 0,
        py::arg("ejones") = py::none(), py::arg("Nsta") = 0);
  m.def("predict_coh_channels", &predict_coh_channels,
        "coherency predict, all channels in one launch (gfx950)",
        py::arg("u"), py::arg("v"), py::arg("w"), py::arg("ll"),
        py::arg("mm"), py::arg("nn1"), py::arg("flux"), py::arg("eX"),
        py::arg("eY"), py::arg("eP"), py::arg("cxi"), py::arg("sxi"),
        py::arg("cphi"), py::arg("sphi"), py::arg("r1"), py::arg("stype"),
        py::arg("cluster_off"), py::arg("freqs"), py::arg("fdelta2"),
        py::arg("tdelta"), py::arg("mean") = false,
        py::arg("beam") = py::none(), py::arg("ejones") = py::none(),
        py::arg("pairs") = py::none(), py::arg("Nbase") = 0,
        py::arg("Nsta") = 0);
  m.def("residuals_multifreq", &residuals_multifreq,
        "predict and subtract, all channels in one launch (gfx950)",
        py::arg("x"), py::arg("u"), py::arg("v"), py::arg("w"), py::arg("ll"),
        py::arg("mm"), py::arg("nn1"), py::arg("flux"), py::arg("eX"),
        py::arg("eY"), py::arg("eP"), py::arg("cxi"), py::arg("sxi"),
        py::arg("cphi"), py::arg("sphi"), py::arg("r1"), py::arg("stype"),
        py::arg("cluster_off"), py::arg("freqs"), py::arg("fdelta2"),
        py::arg("tdelta"), py::arg("J"), py::arg("chunk_tab"),
        py::arg("pairs"), py::arg("skip") = py::none(),
        py::arg("beam") = py::none(), py::arg("ejones") = py::none(),
        py::arg("Nsta") = 0);
  m.attr("PREDICT_MF_NF") = PREDICT_MF_NF;
  m.attr("PREDICT_MF_NF_EJ") = PREDICT_MF_NF_EJ;
  m.def("array_beam_gains", &array_beam_gains,
        "station array-factor gains [T, K, N] (gfx950)", py::arg("elem"),
        py::arg("nelem"), py::arg("du"), py::arg("below"), py::arg("kf"));
  m.def("station_beam_gains", &station_beam_gains,
        "single- or two-stage station beam gains [F, T, K, N] (gfx950)",
        py::arg("elem"), py::arg("nelem"), py::arg("du"), py::arg("below"),
        py::arg("kf"), py::arg("tile") = py::none(),
        py::arg("du_tile") = py::none());
  m.def("element_jones", &element_jones,
        "dipole element E-Jones [F, D, 2, 2] (gfx950)", py::arg("az"),
        py::arg("el"), py::arg("coef"), py::arg("preamble"), py::arg("M"),
        py::arg("beta"));
  m.attr("ELEMENT_BEAM_MAX_M") = ELEMENT_BEAM_MAX_M;
  m.def("jtj_jtr", &jtj_jtr, "fused JtJ/Jtr assembly (gfx950)");
  m.def("model_cost", &model_cost, "per-chunk model cost (gfx950)");
  m.def("apply_jones", &apply_jones, "model apply / residual (gfx950)");
}
