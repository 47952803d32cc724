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

// The one tensor check: contiguous, of dtype ty, on the device dev and,
// with n >= 0, of n elements. Dimensions and shapes stay with the caller.
static bool on_dev(const torch::Tensor& t, const torch::Device& dev,
                   torch::ScalarType ty, int64_t n = -1) {
  return t.is_cuda() && t.device() == dev && t.scalar_type() == ty &&
         t.is_contiguous() && (n < 0 || t.numel() == n);
}

// The kernels read 2x2 matrices as two 16-byte loads.
static void check_aligned16(std::initializer_list<const torch::Tensor*> ts,
                            const char* names) {
  for (const torch::Tensor* t : ts)
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, names,
                " must be 16-byte aligned");
}

// u, v, w: [R] float64 on one device, contiguous
static RowsUVW rows_uvw(const torch::Tensor& u, const torch::Tensor& v,
                        const torch::Tensor& w) {
  TORCH_CHECK(u.is_cuda() && u.dim() == 1, "u must be a device tensor [R]");
  for (const torch::Tensor* t : {&u, &v, &w})
    TORCH_CHECK(on_dev(*t, u.device(), torch::kDouble, u.size(0)),
                "u, v, w must be contiguous [R] float64 on one device");
  RowsUVW rows = {};
  rows.u = dp(u); rows.v = dp(v); rows.w = dp(w);
  rows.R = (int)u.size(0);
  return rows;
}

// The rows of the all-channels entry points: at least one, below 2^31.
static RowsUVW rows_mf(const torch::Tensor& u, const torch::Tensor& v,
                       const torch::Tensor& w) {
  TORCH_CHECK(u.dim() == 1 && u.size(0) >= 1 &&
              u.size(0) < (int64_t(1) << 31), "rows out of range");
  return rows_uvw(u, v, w);
}

// A record is a Python dict from field name to tensor, described by one
// table of rows (name, dtype, length kind, where the pointer goes).
enum Len {
  COUNT,      // n elements; the first row of a table sets n = size(0)
  COUNT1,     // n + 1 elements
  PREFIX,     // one-dimensional [M + 1]: its own length sets M
  FREE        // any length; the record's function checks the shape
};

template <class Rec>
struct Field {
  const char* name;
  torch::ScalarType ty;
  Len len;
  void (*set)(Rec&, const void*);
};

#define FIELD(Rec, key, member, ty, len)                    \
  {#key, ty, len, [](Rec& r, const void* p) {               \
     r.member = static_cast<decltype(r.member)>(p); }}

// Fills rec from the dict d by the table `fields`: every field present, on
// dev, of its dtype, contiguous and of its length, and no key besides them.
// Returns n.
template <class Rec, size_t NF>
static int64_t read_record(const char* what, const py::dict& d,
                           const Field<Rec> (&fields)[NF],
                           const torch::Device& dev, Rec& rec) {
  int64_t n = -1;
  for (const Field<Rec>& f : fields) {
    PyObject* item = PyDict_GetItemString(d.ptr(), f.name);   // borrowed
    TORCH_CHECK(item != nullptr, what, " lacks the field ", f.name);
    const torch::Tensor t = py::cast<torch::Tensor>(py::handle(item));
    if (n < 0) {
      TORCH_CHECK(t.dim() >= 1, what, ".", f.name, " must be [n]");
      n = t.size(0);
    }
    const int64_t want = f.len == COUNT ? n : f.len == COUNT1 ? n + 1 : -1;
    TORCH_CHECK(on_dev(t, dev, f.ty, want) &&
                (f.len != PREFIX || (t.dim() == 1 && t.size(0) >= 1)),
                what, ".", f.name, " must be contiguous ", f.ty,
                f.len == PREFIX ? " [M + 1]" : "", want < 0 ? "" : " with ",
                want < 0 ? "" : std::to_string(want).c_str(),
                want < 0 ? "" : " elements", " on the device of u");
    f.set(rec, t.data_ptr());
  }
  if (d.size() != NF)
    for (auto kv : d) {
      const std::string key = py::str(kv.first);
      bool known = false;
      for (const Field<Rec>& f : fields) known = known || key == f.name;
      TORCH_CHECK(known, what, " has the unknown field ", key);
    }
  return n;
}

// hip_host.GPUPack.record: what k_predict_coh reads per source, K sources in M
// clusters. The fluxes and r1 change per call (set_flux).
static const Field<SourceArrays> SOURCE_FIELDS[] = {
  FIELD(SourceArrays, ll, ll, torch::kDouble, COUNT),
  FIELD(SourceArrays, mm, mm, torch::kDouble, COUNT),
  FIELD(SourceArrays, nn1, nn1, torch::kDouble, COUNT),
  FIELD(SourceArrays, eX, eX, torch::kFloat, COUNT),
  FIELD(SourceArrays, eY, eY, torch::kFloat, COUNT),
  FIELD(SourceArrays, eP, eP, torch::kFloat, COUNT),
  FIELD(SourceArrays, cxi, cxi, torch::kFloat, COUNT),
  FIELD(SourceArrays, sxi, sxi, torch::kFloat, COUNT),
  FIELD(SourceArrays, cphi, cphi, torch::kFloat, COUNT),
  FIELD(SourceArrays, sphi, sphi, torch::kFloat, COUNT),
  FIELD(SourceArrays, stype, stype, torch::kInt, COUNT),
  FIELD(SourceArrays, cluster_off, cluster_off, torch::kInt, PREFIX),
};

// The caller guarantees that cluster_off is non-decreasing from 0 to K.
static SourceArrays source_arrays(const py::dict& src, const torch::Tensor& u,
                                  int64_t& K) {
  SourceArrays s = {};
  K = read_record("src", src, SOURCE_FIELDS, u.device(), s);
  s.M = (int)py::cast<torch::Tensor>(src["cluster_off"]).size(0) - 1;
  return s;
}

// hip_host.ShapeletTable.record: the mode table of the shapelet kernels,
// S entries. flux and r1 change per call.
static const Field<ShapeletTabMF> SHAPELET_FIELDS[] = {
  FIELD(ShapeletTabMF, src, t.src, torch::kInt, COUNT),
  FIELD(ShapeletTabMF, cluster, t.cluster, torch::kInt, COUNT),
  FIELD(ShapeletTabMF, n0, t.n0, torch::kInt, COUNT),
  FIELD(ShapeletTabMF, beta, t.beta, torch::kFloat, COUNT),
  FIELD(ShapeletTabMF, off, t.off, torch::kInt, COUNT1),
  FIELD(ShapeletTabMF, coef, t.coef, torch::kFloat, FREE),
  FIELD(ShapeletTabMF, cxi, t.cxi, torch::kFloat, COUNT),
  FIELD(ShapeletTabMF, sxi, t.sxi, torch::kFloat, COUNT),
  FIELD(ShapeletTabMF, cphi, t.cphi, torch::kFloat, COUNT),
  FIELD(ShapeletTabMF, sphi, t.sphi, torch::kFloat, COUNT),
  FIELD(ShapeletTabMF, psign, t.psign, torch::kFloat, COUNT),
  FIELD(ShapeletTabMF, a, t.a, torch::kFloat, COUNT),
  FIELD(ShapeletTabMF, b, t.b, torch::kFloat, COUNT),
  FIELD(ShapeletTabMF, ceP, t.ceP, torch::kFloat, COUNT),
  FIELD(ShapeletTabMF, seP, t.seP, torch::kFloat, COUNT),
  FIELD(ShapeletTabMF, ll, t.ll, torch::kDouble, COUNT),
  FIELD(ShapeletTabMF, mm, t.mm, torch::kDouble, COUNT),
  FIELD(ShapeletTabMF, nn1, t.nn1, torch::kDouble, COUNT),
  FIELD(ShapeletTabMF, rec, t.rec, torch::kFloat, FREE),
  FIELD(ShapeletTabMF, entry_off, entry_off, torch::kInt, PREFIX),
};

// The single-channel kernel reads tab.t alone. The caller guarantees that
// entry_off is non-decreasing from 0 to S and that src holds source indices
// below K.
static ShapeletTabMF shapelet_tab(const py::dict& tab, const torch::Tensor& u) {
  ShapeletTabMF s = {};
  s.t.S = (int)read_record("tab", tab, SHAPELET_FIELDS, u.device(), s);
  const torch::Tensor rec = py::cast<torch::Tensor>(tab["rec"]);
  TORCH_CHECK(rec.dim() == 2 && rec.size(0) == 2, "rec must be [2, max n0]");
  s.t.nmax = (int)rec.size(1);
  s.M = (int)py::cast<torch::Tensor>(tab["entry_off"]).size(0) - 1;
  return s;
}

// The table of the all-channels shapelet kernels: at least one entry and
// one cluster.
static ShapeletTabMF shapelet_tab_mf(const py::dict& tab,
                                     const torch::Tensor& u) {
  const ShapeletTabMF s = shapelet_tab(tab, u);
  TORCH_CHECK(s.t.S >= 1, "the shapelet table is empty");
  TORCH_CHECK(s.M >= 1, "entry_off must be contiguous [M + 1] int32");
  return s;
}

// The per-call arrays of the single-channel entry points: flux [4, n]
// float32 (I, Q, U, V rows) and r1 [n] float32, n sources or table entries.
static void check_flux_r1(const torch::Tensor& flux, const torch::Tensor& r1,
                          int64_t n, const torch::Device& dev) {
  TORCH_CHECK(on_dev(flux, dev, torch::kFloat, 4 * n) && flux.dim() == 2 &&
              flux.size(0) == 4, "flux must be contiguous [4, ", n,
              "] float32");
  TORCH_CHECK(on_dev(r1, dev, torch::kFloat, n), "r1 must be contiguous [", n,
              "] float32");
}

// The per-call arrays of the all-channels entry points: freqs [F] float64,
// the flux stack [F, 4, n] float32 (I, Q, U, V rows per channel) and r1 [n].
static Channels channels(const torch::Tensor& freqs, const torch::Tensor& flux,
                         const torch::Tensor& r1, int64_t n, double fdelta2,
                         double tdelta, const torch::Device& dev) {
  TORCH_CHECK(on_dev(freqs, dev, torch::kDouble) && freqs.dim() == 1 &&
              freqs.size(0) >= 1, "freqs must be contiguous [F] float64, "
              "F >= 1");
  const int64_t F = freqs.size(0);
  TORCH_CHECK(on_dev(flux, dev, torch::kFloat) && flux.dim() == 3 &&
              flux.size(0) == F && flux.size(1) == 4 && flux.size(2) == n,
              "flux must be contiguous [F, 4, ", n, "] float32");
  TORCH_CHECK(on_dev(r1, dev, torch::kFloat, n), "r1 must be contiguous [", n,
              "] float32");
  Channels ch = {};
  ch.freqs = dp(freqs);
  ch.F = (int)F;
  ch.fdelta2 = fdelta2;
  ch.tdelta = tdelta;
  ch.flux_stride = 4 * n;
  return ch;
}

// sI..sV are the rows of flux [4, K], or of channel 0 of [F, 4, K].
static void set_flux(SourceArrays& s, const torch::Tensor& flux,
                     const torch::Tensor& r1, int64_t K) {
  s.sI = fp(flux); s.sQ = s.sI + K; s.sU = s.sI + 2 * K; s.sV = s.sI + 3 * K;
  s.r1 = fp(r1);
}

// The pair table [Nbase, 2] int32 that a beam is indexed through.
static const int* beam_pairs(const c10::optional<torch::Tensor>& pairs,
                             int64_t Nbase, const torch::Device& dev) {
  TORCH_CHECK(pairs.has_value() && Nbase > 0,
              "beam and ejones need the station-pair table and Nbase");
  TORCH_CHECK(on_dev(*pairs, dev, torch::kInt, 2 * Nbase),
              "pairs must be contiguous [Nbase, 2] int32");
  return ip(*pairs);
}

// The optional station beam of both single-channel entry points: beam
// [T, K, N] float32, pairs [Nbase, 2] int32 and ejones [T, K, NE, 2, 2]
// complex64, checked against the R rows. The kernels index all three by
// timeslot, source and station with no bounds of their own, and read pairs
// on every row with either buffer. Nsta_ej is the station count that ejones
// goes with (beam brings its own).
static BeamArgs beam_args(
    const c10::optional<torch::Tensor>& beam,
    const c10::optional<torch::Tensor>& pairs,
    const c10::optional<torch::Tensor>& ejones, int64_t R, int64_t Nbase,
    int64_t Nsta_ej, const torch::Device& dev) {
  BeamArgs a = {};
  if (!beam.has_value() && !ejones.has_value()) return a;
  a.pairs = beam_pairs(pairs, Nbase, dev);
  a.Nbase = (int)Nbase;
  if (beam.has_value()) {
    TORCH_CHECK(on_dev(*beam, dev, torch::kFloat) && beam->dim() == 3,
                "beam must be contiguous [T, K, N] float32");
    TORCH_CHECK(R <= beam->size(0) * Nbase,
                "beam has too few timeslots for the rows");
    a.beam = fp(*beam);
    a.Ktot = (int)beam->size(1);
    a.Nsta = (int)beam->size(2);
  }
  if (ejones.has_value()) {
    const torch::Tensor& e = *ejones;
    TORCH_CHECK(on_dev(e, dev, torch::kComplexFloat) && e.dim() == 5 &&
                e.size(3) == 2 && e.size(4) == 2,
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

// Coherencies [M, R, 4] complex64 of the pack record `src` at one channel
// (k_predict_coh, with ejones k_predict_coh_ej): flux [4, K], r1 [K].
torch::Tensor predict_coh(
    torch::Tensor u, torch::Tensor v, torch::Tensor w, py::dict src_rec,
    torch::Tensor flux, torch::Tensor r1, double freq, double fdelta2,
    double tdelta, c10::optional<torch::Tensor> beam,
    c10::optional<torch::Tensor> pairs, int64_t Nbase,
    c10::optional<torch::Tensor> ejones, int64_t Nsta_ej) {
  const RowsUVW rows = rows_uvw(u, v, w);
  int64_t K;
  SourceArrays src = source_arrays(src_rec, u, K);
  check_flux_r1(flux, r1, K, u.device());
  set_flux(src, flux, r1, K);
  const BeamArgs bm = beam_args(beam, pairs, ejones, rows.R, Nbase, Nsta_ej,
                                u.device());
  auto out = torch::empty({src.M, rows.R, 4},
      torch::dtype(torch::kComplexFloat).device(u.device()));
  CHECK_HIP(launch_predict_coh(rows, src, {freq, fdelta2, tdelta}, bm,
                               cptr(out), cur_stream()));
  return out;
}

// Adds the shapelet sources of the table record `tab` into `out` [M, R, 4]
// complex64, in place, on the current stream: flux [4, S], r1 [S].
void shapelet_coh_add(
    torch::Tensor out, torch::Tensor u, torch::Tensor v, torch::Tensor w,
    py::dict tab_rec, torch::Tensor flux, torch::Tensor r1, double freq,
    double fdelta2, double tdelta, c10::optional<torch::Tensor> beam,
    c10::optional<torch::Tensor> pairs, int64_t Nbase,
    c10::optional<torch::Tensor> ejones, int64_t Nsta_ej) {
  const RowsUVW rows = rows_uvw(u, v, w);
  TORCH_CHECK(on_dev(out, u.device(), torch::kComplexFloat) &&
              out.dim() == 3 && out.size(1) == rows.R && out.size(2) == 4,
              "out must be contiguous [M, R, 4] complex64");
  ShapeletTab tab = shapelet_tab(tab_rec, u).t;
  check_flux_r1(flux, r1, tab.S, u.device());
  tab.flux = fp(flux); tab.r1 = fp(r1);
  const BeamArgs bm = beam_args(beam, pairs, ejones, rows.R, Nbase, Nsta_ej,
                                u.device());
  CHECK_HIP(launch_shapelet_coh(rows, tab, {freq, fdelta2, tdelta}, bm,
                                cptr(out), cur_stream()));
}

// The optional station beam of the all-channels entry points: beam
// [F, T, Ke, N] float32, ejones [F, T, Ke, NE, 2, 2] complex64 and pairs
// [Nbase, 2] int32, checked against the F channels, R rows and K sources.
// The kernels index the buffers by channel, timeslot, source and station
// with no bounds of their own; the caller guarantees pair entries below the
// station count (negative ones only where the kernel keeps x). Nsta_ej is
// the station count that ejones goes with (beam brings its own).
static BeamChannels beam_channels(
    const c10::optional<torch::Tensor>& beam,
    const c10::optional<torch::Tensor>& ejones,
    const c10::optional<torch::Tensor>& pairs, int64_t Nbase,
    int64_t Nsta_ej, int64_t R, int64_t F, int64_t K,
    const torch::Device& dev) {
  BeamChannels b = {};
  if (!beam.has_value() && !ejones.has_value()) return b;
  b.pairs = beam_pairs(pairs, Nbase, dev);
  TORCH_CHECK(R % Nbase == 0, "rows must be T * Nbase");
  const int64_t T = R / Nbase;
  b.Nbase = (int)Nbase;
  b.T = (int)T;
  auto fits = [](int64_t n) { return n >= 1 && n < (int64_t(1) << 31); };
  if (beam.has_value()) {
    const torch::Tensor& g = *beam;
    TORCH_CHECK(on_dev(g, dev, torch::kFloat) && g.dim() == 4,
                "beam must be contiguous [F, T, K, N] float32");
    TORCH_CHECK(g.size(0) == F && g.size(1) == T,
                "beam must hold the F channels and T timeslots of the rows");
    TORCH_CHECK(g.size(2) >= K && fits(g.size(2)) && fits(g.size(3)),
                "beam covers fewer sources than the pack");
    b.beam = fp(g);
    b.Ktot = (int)g.size(2);
    b.Nsta = (int)g.size(3);
  }
  if (ejones.has_value()) {
    const torch::Tensor& e = *ejones;
    TORCH_CHECK(on_dev(e, dev, torch::kComplexFloat) && e.dim() == 6 &&
                e.size(4) == 2 && e.size(5) == 2,
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

// J [Mt, N, 4] complex64 packed solutions, chunk_tab [M, T] and pairs
// [Nbase, 2] int32 on dev, for R == T * Nbase rows. The caller guarantees
// chunk ids below Mt and pair entries below N.
static void check_solution_tables(
    const torch::Tensor& J, const torch::Tensor& chunk_tab,
    const torch::Tensor& pairs, int64_t M, int64_t R,
    const torch::Device& dev) {
  TORCH_CHECK(on_dev(J, dev, torch::kComplexFloat) && J.dim() == 3 &&
              J.size(0) >= 1 && J.size(1) >= 1 && J.size(2) == 4,
              "J must be contiguous [Mt, N, 4] complex64");
  TORCH_CHECK(on_dev(chunk_tab, dev, torch::kInt) && chunk_tab.dim() == 2 &&
              chunk_tab.size(0) == M && chunk_tab.size(1) >= 1,
              "chunk_tab must be contiguous [M, T] int32");
  TORCH_CHECK(on_dev(pairs, dev, torch::kInt) && pairs.dim() == 2 &&
              pairs.size(0) >= 1 && pairs.size(1) == 2,
              "pairs must be contiguous [Nbase, 2] int32");
  TORCH_CHECK(chunk_tab.size(1) * pairs.size(0) == R &&
              R < (int64_t(1) << 31), "rows must be T * Nbase, below 2^31");
}

// What the two residual entry points take besides the predict arguments:
// the tables of check_solution_tables and skip [M] int32 or none. x is left
// to the caller.
static ResidualArgs residual_args(
    const torch::Tensor& J, const torch::Tensor& chunk_tab,
    const torch::Tensor& pairs, const c10::optional<torch::Tensor>& skip,
    int64_t M, int64_t R, const torch::Device& dev) {
  check_solution_tables(J, chunk_tab, pairs, M, R, dev);
  ResidualArgs res = {};
  res.J = ccptr(J);
  res.chunk_tab = ip(chunk_tab);
  res.pairs = ip(pairs);
  if (skip.has_value()) {
    TORCH_CHECK(on_dev(*skip, dev, torch::kInt, M),
                "skip must be contiguous [M] int32");
    res.skip = ip(*skip);
  }
  res.Nbase = (int)pairs.size(0);
  res.T = (int)chunk_tab.size(1);
  res.N = (int)J.size(1);
  return res;
}

// Coherencies of all F channels in one launch (k_predict_coh_mf):
// [F, M, R, 4] complex64, or with mean their channel mean [M, R, 4]
// (k_predict_coh_mean); with beam and/or ejones the _bm / _ej kernels. src is
// the pack record, flux [F, 4, K], r1 [K].
torch::Tensor predict_coh_channels(
    torch::Tensor u, torch::Tensor v, torch::Tensor w, py::dict src_rec,
    torch::Tensor flux, torch::Tensor r1, torch::Tensor freqs, double fdelta2,
    double tdelta, bool mean, c10::optional<torch::Tensor> beam,
    c10::optional<torch::Tensor> ejones, c10::optional<torch::Tensor> pairs,
    int64_t Nbase, int64_t Nsta_ej) {
  const torch::Device dev = u.device();
  const RowsUVW rows = rows_mf(u, v, w);
  int64_t K;
  SourceArrays src = source_arrays(src_rec, u, K);
  const Channels ch = channels(freqs, flux, r1, K, fdelta2, tdelta, dev);
  set_flux(src, flux, r1, K);
  const BeamChannels bm = beam_channels(beam, ejones, pairs, Nbase, Nsta_ej,
                                        rows.R, ch.F, K, dev);
  auto copts = torch::dtype(torch::kComplexFloat).device(dev);
  auto out = mean ? torch::empty({src.M, rows.R, 4}, copts)
                  : torch::empty({ch.F, src.M, rows.R, 4}, copts);
  CHECK_HIP(launch_predict_coh_mf(rows, src, ch, bm, mean ? 1 : 0, cptr(out),
                                  cur_stream()));
  return out;
}

// x - sum over clusters with skip == 0 of J_p C J_q^H for all F channels in
// one launch (k_residual_mf): x [F, R, 4] complex64, the tables of
// residual_args. Returns [F, R, 4]. With beam [F, T, Ke, Nsta] and/or ejones
// [F, T, Ke, NE, 2, 2] the coherencies carry the station beam
// (k_residual_mf_bm / _ej), indexed through the same pairs.
torch::Tensor residuals_multifreq(
    torch::Tensor x, torch::Tensor u, torch::Tensor v, torch::Tensor w,
    py::dict src_rec, torch::Tensor flux, torch::Tensor r1,
    torch::Tensor freqs, double fdelta2, double tdelta, torch::Tensor J,
    torch::Tensor chunk_tab, torch::Tensor pairs,
    c10::optional<torch::Tensor> skip, c10::optional<torch::Tensor> beam,
    c10::optional<torch::Tensor> ejones, int64_t Nsta_ej) {
  const torch::Device dev = u.device();
  const RowsUVW rows = rows_mf(u, v, w);
  int64_t K;
  SourceArrays src = source_arrays(src_rec, u, K);
  const Channels ch = channels(freqs, flux, r1, K, fdelta2, tdelta, dev);
  set_flux(src, flux, r1, K);
  const int64_t R = rows.R, F = ch.F;
  TORCH_CHECK(on_dev(x, dev, torch::kComplexFloat) && x.dim() == 3 &&
              x.size(0) == F && x.size(1) == R && x.size(2) == 4,
              "x must be contiguous [F, R, 4] complex64");
  ResidualArgs res = residual_args(J, chunk_tab, pairs, skip, src.M, R, dev);
  res.x = ccptr(x);
  const BeamChannels bm = beam_channels(beam, ejones, pairs, pairs.size(0),
                                        Nsta_ej, R, F, K, dev);
  auto out = torch::empty({F, R, 4},
      torch::dtype(torch::kComplexFloat).device(dev));
  CHECK_HIP(launch_residual_mf(rows, src, ch, bm, res, cptr(out),
                               cur_stream()));
  return out;
}

// Adds the shapelet sources of all F channels into `out`, what
// predict_coh_channels returned for the same rows, channels, mean and beam
// (k_shapelet_coh_mf / _mean, with beam and/or ejones _bm / _ej): [F, M, R,
// 4] complex64, or with mean [M, R, 4]. In place, on the current stream. tab
// is the table record, flux [F, 4, S], r1 [S]; K is the source count of the
// pack, which beam and ejones must cover.
void shapelet_coh_channels_add(
    torch::Tensor out, torch::Tensor u, torch::Tensor v, torch::Tensor w,
    py::dict tab_rec, torch::Tensor flux, torch::Tensor r1,
    torch::Tensor freqs, double fdelta2, double tdelta, bool mean, int64_t K,
    c10::optional<torch::Tensor> beam, c10::optional<torch::Tensor> ejones,
    c10::optional<torch::Tensor> pairs, int64_t Nbase, int64_t Nsta_ej) {
  const torch::Device dev = u.device();
  const RowsUVW rows = rows_mf(u, v, w);
  ShapeletTabMF tab = shapelet_tab_mf(tab_rec, u);
  const Channels ch = channels(freqs, flux, r1, tab.t.S, fdelta2, tdelta, dev);
  tab.t.flux = fp(flux); tab.t.r1 = fp(r1);
  const int64_t R = rows.R, F = ch.F, M = tab.M;
  TORCH_CHECK(on_dev(out, dev, torch::kComplexFloat,
                     (mean ? 1 : F) * M * R * 4) &&
              out.dim() == (mean ? 3 : 4) && out.size(-2) == R,
              "out must be contiguous [F, M, R, 4] complex64, or [M, R, 4] "
              "with mean");
  const BeamChannels bm = beam_channels(beam, ejones, pairs, Nbase, Nsta_ej,
                                        R, F, K, dev);
  CHECK_HIP(launch_shapelet_coh_mf(rows, tab, ch, bm, mean ? 1 : 0, cptr(out),
                                   cur_stream()));
}

// Subtracts J_p C J_q^H of the shapelet sources of every cluster with
// entries and skip == 0 from `out` [F, R, 4] complex64, what
// residuals_multifreq returned for the same arguments
// (k_shapelet_residual_mf, _bm, _ej). In place, on the current stream; J,
// chunk_tab, pairs, skip and the caller's guarantees as there.
void shapelet_residuals_add(
    torch::Tensor out, torch::Tensor u, torch::Tensor v, torch::Tensor w,
    py::dict tab_rec, torch::Tensor flux, torch::Tensor r1,
    torch::Tensor freqs, double fdelta2, double tdelta, torch::Tensor J,
    torch::Tensor chunk_tab, torch::Tensor pairs,
    c10::optional<torch::Tensor> skip, int64_t K,
    c10::optional<torch::Tensor> beam, c10::optional<torch::Tensor> ejones,
    int64_t Nsta_ej) {
  const torch::Device dev = u.device();
  const RowsUVW rows = rows_mf(u, v, w);
  ShapeletTabMF tab = shapelet_tab_mf(tab_rec, u);
  const Channels ch = channels(freqs, flux, r1, tab.t.S, fdelta2, tdelta, dev);
  tab.t.flux = fp(flux); tab.t.r1 = fp(r1);
  const int64_t R = rows.R, F = ch.F;
  TORCH_CHECK(on_dev(out, dev, torch::kComplexFloat) && out.dim() == 3 &&
              out.size(0) == F && out.size(1) == R && out.size(2) == 4,
              "out must be contiguous [F, R, 4] complex64");
  const ResidualArgs res = residual_args(J, chunk_tab, pairs, skip, tab.M, R,
                                         dev);
  const BeamChannels bm = beam_channels(beam, ejones, pairs, pairs.size(0),
                                        Nsta_ej, R, F, K, dev);
  CHECK_HIP(launch_shapelet_residual_mf(rows, tab, ch, bm, res, cptr(out),
                                        cur_stream()));
}

// The four tensors both beam-gain entry points share: elem [N, Emax, 3]
// float64 on the device, nelem [N] int32 (the caller has checked
// 1 <= nelem <= Emax on the host), du [T, K, 3] float64, below [T, K] uint8.
static void check_beam_geometry(
    const torch::Tensor& elem, const torch::Tensor& nelem,
    const torch::Tensor& du, const torch::Tensor& below) {
  const torch::Device dev = elem.device();
  TORCH_CHECK(on_dev(elem, dev, torch::kDouble) && elem.dim() == 3 &&
              elem.size(2) == 3 && elem.size(1) > 0,
              "elem must be contiguous [N, Emax, 3] float64");
  TORCH_CHECK(on_dev(nelem, dev, torch::kInt, elem.size(0)),
              "nelem must be contiguous [N] int32");
  TORCH_CHECK(on_dev(du, dev, torch::kDouble) && du.dim() == 3 &&
              du.size(2) == 3, "du must be contiguous [T, K, 3] float64");
  TORCH_CHECK(on_dev(below, dev, torch::kByte) && below.dim() == 2 &&
              below.size(0) == du.size(0) && below.size(1) == du.size(1),
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
  const torch::Device dev = elem.device();
  const int64_t N = elem.size(0), Emax = elem.size(1);
  const int64_t T = du.size(0), K = du.size(1);
  TORCH_CHECK(on_dev(kf, dev, torch::kDouble) && kf.dim() == 1,
              "kf must be contiguous [F] float64");
  const int64_t F = kf.size(0);
  TORCH_CHECK(tile.has_value() == du_tile.has_value(),
              "tile and du_tile come together");
  const double* tile_p = nullptr;
  const double* dut_p = nullptr;
  int64_t D = 0;
  if (tile.has_value()) {
    const torch::Tensor& tl = *tile;
    const torch::Tensor& dt = *du_tile;
    TORCH_CHECK(on_dev(tl, dev, torch::kDouble) && tl.dim() == 3 &&
                tl.size(0) == N && tl.size(2) == 3 && tl.size(1) >= 1 &&
                tl.size(1) <= 64,
                "tile must be contiguous [N, D, 3] float64, 1 <= D <= 64");
    TORCH_CHECK(on_dev(dt, dev, torch::kDouble) && dt.dim() == 3 &&
                dt.size(0) == T && dt.size(1) == K && dt.size(2) == 3,
                "du_tile must be contiguous [T, K, 3] float64");
    D = tl.size(1);
    tile_p = tl.data_ptr<double>();
    dut_p = dt.data_ptr<double>();
  }
  auto gain = torch::empty({F, T, K, N},
      torch::dtype(torch::kFloat).device(dev));
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
  const torch::Device dev = az.device();
  TORCH_CHECK(on_dev(az, dev, torch::kDouble) && az.dim() == 1,
              "az must be contiguous [D] float64 on the device");
  TORCH_CHECK(on_dev(el, dev, torch::kDouble) && el.dim() == 1 &&
              el.size(0) == az.size(0),
              "el must be contiguous [D] float64 like az");
  TORCH_CHECK(on_dev(coef, dev, torch::kComplexFloat) && coef.dim() == 3 &&
              coef.size(0) >= 1 && coef.size(1) == 2 &&
              coef.size(2) == Nmodes,
              "coef must be contiguous [F, 2, M(M+1)/2] complex64, F >= 1");
  TORCH_CHECK(on_dev(preamble, dev, torch::kFloat) && preamble.dim() == 1 &&
              preamble.size(0) == Nmodes,
              "preamble must be contiguous [M(M+1)/2] float32");
  const int64_t D = az.size(0), F = coef.size(0);
  TORCH_CHECK(D < (int64_t(1) << 31) && F < (int64_t(1) << 31),
              "too many directions or frequencies");
  auto E = torch::empty({F, D, 2, 2},
      torch::dtype(torch::kComplexFloat).device(dev));
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

std::vector<torch::Tensor> chol_solve_blocked(
    torch::Tensor JtJ, torch::Tensor Jtr, torch::Tensor mu,
    torch::Tensor scratch) {
  return chol_solve_with(launch_chol_blocked, JtJ, Jtr, mu, scratch);
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

// Cost and gradient of the multi-channel LBFGS objective (lbfgs_mf.hip): xs
// [F, R, 4], cohs [F, M, R, 4] and J [Mt, N, 4] complex64, chunk_tab [M, T]
// and pairs [Nbase, 2] int32 with R == T * Nbase, and the index tables of
// hip_host._lbfgs_tables: ext [E, 4], ext_off [Mt + 1], sta_off [N + 1],
// sta_ent. robust_nu <= 0: Gaussian cost. Returns (cost [] float32, grad
// [Mt*N*8] float32). The caller guarantees chunk ids below Mt, pair entries
// below N and tables that match chunk_tab and pairs.
std::vector<torch::Tensor> lbfgs_cost_grad_channels(
    torch::Tensor xs, torch::Tensor cohs, torch::Tensor J,
    torch::Tensor chunk_tab, torch::Tensor pairs, torch::Tensor ext,
    torch::Tensor ext_off, torch::Tensor sta_off, torch::Tensor sta_ent,
    double robust_nu) {
  const torch::Device dev = xs.device();
  TORCH_CHECK(on_dev(xs, dev, torch::kComplexFloat) && xs.dim() == 3 &&
              xs.size(0) >= 1 && xs.size(1) >= 1 && xs.size(2) == 4,
              "xs must be contiguous [F, R, 4] complex64 on the device");
  const int64_t F = xs.size(0), R = xs.size(1);
  TORCH_CHECK(on_dev(cohs, dev, torch::kComplexFloat) && cohs.dim() == 4 &&
              cohs.size(0) == F && cohs.size(1) >= 1 && cohs.size(2) == R &&
              cohs.size(3) == 4,
              "cohs must be contiguous [F, M, R, 4] complex64");
  const int64_t M = cohs.size(1);
  check_solution_tables(J, chunk_tab, pairs, M, R, dev);
  const int64_t Mt = J.size(0), N = J.size(1);
  const int64_t T = chunk_tab.size(1), Nbase = pairs.size(0);
  TORCH_CHECK(on_dev(ext, dev, torch::kInt) && ext.dim() == 2 &&
              ext.size(0) >= 1 && ext.size(1) == 4,
              "ext must be contiguous [E, 4] int32");
  const int64_t E = ext.size(0);
  TORCH_CHECK(on_dev(ext_off, dev, torch::kInt, Mt + 1),
              "ext_off must be contiguous [Mt + 1] int32");
  TORCH_CHECK(on_dev(sta_off, dev, torch::kInt, N + 1),
              "sta_off must be contiguous [N + 1] int32");
  TORCH_CHECK(on_dev(sta_ent, dev, torch::kInt) &&
              sta_ent.numel() <= 2 * Nbase,
              "sta_ent must be contiguous int32, at most 2 * Nbase entries");
  TORCH_CHECK(E < (int64_t(1) << 31) / Nbase && Mt * N < (int64_t(1) << 28),
              "too many extents or parameters");
  check_aligned16({&xs, &cohs, &J}, "xs, cohs and J");
  LbfgsMfArgs a = {};
  a.xs = ccptr(xs); a.cohs = ccptr(cohs); a.J = ccptr(J);
  a.pairs = ip(pairs); a.chunk_tab = ip(chunk_tab);
  a.ext = ip(ext); a.ext_off = ip(ext_off);
  a.sta_off = ip(sta_off); a.sta_ent = ip(sta_ent);
  a.F = (int)F; a.M = (int)M; a.T = (int)T; a.Nbase = (int)Nbase;
  a.N = (int)N; a.Mt = (int)Mt; a.E = (int)E;
  a.nu = (float)robust_nu;
  auto fopts = torch::dtype(torch::kFloat).device(dev);
  auto copts = torch::dtype(torch::kComplexFloat).device(dev);
  auto sres = torch::empty({F, R, 4}, copts);
  auto slots = torch::empty({E, Nbase, 8}, copts);
  auto cpart = torch::empty({F * ((R + LBFGS_MF_TB - 1) / LBFGS_MF_TB)},
                            fopts);
  auto cost = torch::empty({}, fopts);
  auto grad = torch::empty({Mt * N * 8}, fopts);
  CHECK_HIP(launch_lbfgs_mf(a, cptr(sres), cptr(slots),
                            cpart.data_ptr<float>(), cost.data_ptr<float>(),
                            grad.data_ptr<float>(), cur_stream()));
  return {cost, grad};
}

// Joint cross-cluster normal equations (joint_jtj.hip): x [R, 4], cohs
// [M, R, 4] and J [Mt, N, 4] complex64, optional wts [R] float32, pairs
// [Nbase, 2] and chunk_tab [M, T] int32 with R == T * Nbase, and the tables
// of hip_host._joint_tables (pieces, etab, gtab, cbin, sdst, gdst, cpos) and
// hip_host._lbfgs_stations (sta_off, sta_ent). nblk blocks of Mt / nblk
// chunks each: returns (H [nblk, ld, ld], g [nblk, ld], cost [nbin]) with
// ld = 8 N Mt / nblk, or with cost_only (cost [nbin],) at this J. The caller
// guarantees chunk ids below Mt, pair entries below N and tables that match
// chunk_tab and pairs.
std::vector<torch::Tensor> joint_jtj(
    torch::Tensor x, torch::Tensor cohs, torch::Tensor J,
    c10::optional<torch::Tensor> wts, torch::Tensor pairs,
    torch::Tensor chunk_tab, torch::Tensor pieces, torch::Tensor etab,
    torch::Tensor gtab, torch::Tensor cbin, torch::Tensor sdst,
    torch::Tensor gdst, torch::Tensor cpos, torch::Tensor sta_off,
    torch::Tensor sta_ent, int64_t nblk, int64_t nbin, bool cost_only) {
  const torch::Device dev = x.device();
  TORCH_CHECK(on_dev(x, dev, torch::kComplexFloat) && x.dim() == 2 &&
              x.size(0) >= 1 && x.size(1) == 4,
              "x must be contiguous [R, 4] complex64 on the device");
  const int64_t R = x.size(0);
  TORCH_CHECK(on_dev(cohs, dev, torch::kComplexFloat) && cohs.dim() == 3 &&
              cohs.size(0) >= 1 && cohs.size(1) == R && cohs.size(2) == 4,
              "cohs must be contiguous [M, R, 4] complex64");
  const int64_t M = cohs.size(0);
  TORCH_CHECK(!wts.has_value() || on_dev(*wts, dev, torch::kFloat, R),
              "weights must be contiguous [R] float32");
  check_solution_tables(J, chunk_tab, pairs, M, R, dev);
  const int64_t Mt = J.size(0), N = J.size(1);
  const int64_t T = chunk_tab.size(1), Nbase = pairs.size(0);
  TORCH_CHECK(on_dev(pieces, dev, torch::kInt) && pieces.dim() == 2 &&
              pieces.size(0) >= 1 && pieces.size(1) == 2,
              "pieces must be contiguous [E, 2] int32");
  const int64_t E = pieces.size(0), ntri = M * (M + 1) / 2;
  TORCH_CHECK(on_dev(cbin, dev, torch::kInt, E),
              "cbin must be contiguous [E] int32");
  TORCH_CHECK(nblk >= 1 && Mt % nblk == 0 && nbin >= 1,
              "Mt must be a multiple of the block count");
  TORCH_CHECK(Mt * N < (int64_t(1) << 27), "too many parameters");
  check_aligned16({&x, &cohs, &J}, "x, cohs and J");
  JointJtjArgs a = {};
  a.x = ccptr(x); a.cohs = ccptr(cohs); a.J = ccptr(J);
  a.wts = wts.has_value() ? wts->data_ptr<float>() : nullptr;
  a.pairs = ip(pairs); a.chunk_tab = ip(chunk_tab); a.pieces = ip(pieces);
  a.cbin = ip(cbin);
  a.M = (int)M; a.T = (int)T; a.Nbase = (int)Nbase; a.N = (int)N;
  a.Mt = (int)Mt; a.E = (int)E; a.nbin = (int)nbin;
  a.ld = 8 * N * (Mt / nblk);
  auto fopts = torch::dtype(torch::kFloat).device(dev);
  auto copts = torch::dtype(torch::kComplexFloat).device(dev);
  auto PC = torch::empty({Nbase, E}, fopts);
  auto cost = torch::empty({nbin}, fopts);
  if (cost_only) {
    CHECK_HIP(launch_joint_cost(a, PC.data_ptr<float>(),
                                cost.data_ptr<float>(), cur_stream()));
    return {cost};
  }
  TORCH_CHECK(on_dev(etab, dev, torch::kInt, E * ntri),
              "etab must be contiguous [E, M(M+1)/2] int32");
  TORCH_CHECK(on_dev(gtab, dev, torch::kInt, E * M),
              "gtab must be contiguous [E, M] int32");
  TORCH_CHECK(on_dev(sdst, dev, torch::kInt) && sdst.dim() == 2 &&
              sdst.size(0) >= 1 && sdst.size(1) == 2,
              "sdst must be contiguous [D, 2] int32");
  TORCH_CHECK(on_dev(gdst, dev, torch::kInt) && gdst.numel() >= 1 &&
              gdst.numel() <= Mt, "gdst must be contiguous [G] int32");
  TORCH_CHECK(on_dev(cpos, dev, torch::kInt, 2 * Mt),
              "cpos must be contiguous [Mt, 2] int32");
  TORCH_CHECK(on_dev(sta_off, dev, torch::kInt, N + 1),
              "sta_off must be contiguous [N + 1] int32");
  TORCH_CHECK(on_dev(sta_ent, dev, torch::kInt) &&
              sta_ent.numel() <= 2 * Nbase,
              "sta_ent must be contiguous int32, at most 2 * Nbase entries");
  a.etab = ip(etab); a.gtab = ip(gtab); a.sdst = ip(sdst); a.gdst = ip(gdst);
  a.cpos = ip(cpos); a.sta_off = ip(sta_off); a.sta_ent = ip(sta_ent);
  a.D = (int)sdst.size(0); a.G = (int)gdst.numel();
  auto PE = torch::empty({Nbase, (int64_t)a.D, 2, 4}, copts);
  auto PG = torch::empty({Nbase, (int64_t)a.G, 2, 4}, copts);
  auto H = torch::zeros({nblk, (int64_t)a.ld, (int64_t)a.ld}, fopts);
  auto g = torch::zeros({nblk, (int64_t)a.ld}, fopts);
  CHECK_HIP(launch_joint_jtj(a, cptr(PE), cptr(PG), PC.data_ptr<float>(),
                             H.data_ptr<float>(), g.data_ptr<float>(),
                             cost.data_ptr<float>(), cur_stream()));
  return {H, g, cost};
}

// The RTR truncated-CG inner solve (rtr_tcg.hip): JtJ [n, P, P], Jtr [n, P],
// iw [N] and delta [n] float32, J [n, N, 2, 2] complex64, P = 8 N. Returns
// (g, eta, Heta [n, N, 2, 2] complex64, stats [n, 4] float32).
std::vector<torch::Tensor> rtr_tcg(
    torch::Tensor JtJ, torch::Tensor Jtr, torch::Tensor J, torch::Tensor iw,
    torch::Tensor delta, int64_t maxit, double kappa) {
  const torch::Device dev = JtJ.device();
  TORCH_CHECK(on_dev(J, dev, torch::kComplexFloat) && J.dim() == 4 &&
              J.size(0) >= 1 && J.size(2) == 2 && J.size(3) == 2,
              "J must be contiguous [n, N, 2, 2] complex64 on the device");
  const int64_t n = J.size(0), N = J.size(1), P = 8 * N;
  TORCH_CHECK(N >= 2 && P <= RTR_TCG_MAXP && n < (int64_t(1) << 31),
              "rtr_tcg takes 2 <= N <= ", RTR_TCG_MAXP / 8, " stations");
  TORCH_CHECK(on_dev(JtJ, dev, torch::kFloat) && JtJ.dim() == 3 &&
              JtJ.size(0) == n && JtJ.size(1) == P && JtJ.size(2) == P,
              "JtJ must be contiguous [n, 8N, 8N] float32");
  TORCH_CHECK(on_dev(Jtr, dev, torch::kFloat) && Jtr.dim() == 2 &&
              Jtr.size(0) == n && Jtr.size(1) == P,
              "Jtr must be contiguous [n, 8N] float32");
  TORCH_CHECK(on_dev(iw, dev, torch::kFloat) && iw.dim() == 1 &&
              iw.size(0) == N, "iw must be contiguous [N] float32");
  TORCH_CHECK(on_dev(delta, dev, torch::kFloat) && delta.dim() == 1 &&
              delta.size(0) == n, "delta must be contiguous [n] float32");
  TORCH_CHECK(maxit >= 0 && maxit < (int64_t(1) << 24),
              "maxit must be in 0 .. 2^24");
  check_aligned16({&JtJ, &Jtr, &J}, "JtJ, Jtr and J");
  RtrTcgArgs a = {};
  a.JtJ = fp(JtJ); a.Jtr = fp(Jtr); a.J = ccptr(J); a.iw = fp(iw);
  a.delta = fp(delta);
  a.n = (int)n; a.N = (int)N; a.maxit = (int)maxit; a.kappa = (float)kappa;
  auto g = torch::empty_like(J), eta = torch::empty_like(J),
       Heta = torch::empty_like(J);
  auto stats = torch::empty({n, 4}, JtJ.options());
  CHECK_HIP(launch_rtr_tcg(a, cptr(g), cptr(eta), cptr(Heta),
                           stats.data_ptr<float>(), cur_stream()));
  return {g, eta, Heta, stats};
}

// The influence-map leverage of every cluster (leverage.hip): cohs [M, R, 4]
// and J [Mt, N, 4] complex64, Hinv [Mt, 8N, 8N] float64, optional wts [R]
// float64, chunk_tab [M, T] and pairs [Nbase, 2] int32 with R == T * Nbase,
// pieces [E, 4] int32 (ci, c, t0, t1) from hip_host._lbfgs_extents. Returns
// lev [M, R] float64. The caller guarantees chunk ids below Mt, pair entries
// below N and pieces that cover chunk_tab.
torch::Tensor leverage_rows(
    torch::Tensor cohs, torch::Tensor J, torch::Tensor Hinv,
    c10::optional<torch::Tensor> wts, torch::Tensor chunk_tab,
    torch::Tensor pairs, torch::Tensor pieces) {
  const torch::Device dev = cohs.device();
  TORCH_CHECK(on_dev(cohs, dev, torch::kComplexFloat) && cohs.dim() == 3 &&
              cohs.size(0) >= 1 && cohs.size(1) >= 1 && cohs.size(2) == 4,
              "cohs must be contiguous [M, R, 4] complex64 on the device");
  const int64_t M = cohs.size(0), R = cohs.size(1);
  check_solution_tables(J, chunk_tab, pairs, M, R, dev);
  const int64_t Mt = J.size(0), N = J.size(1);
  TORCH_CHECK(on_dev(Hinv, dev, torch::kDouble) && Hinv.dim() == 3 &&
              Hinv.size(0) == Mt && Hinv.size(1) == 8 * N &&
              Hinv.size(2) == 8 * N,
              "Hinv must be contiguous [Mt, 8N, 8N] float64 for the Mt chunks "
              "of J");
  TORCH_CHECK(!wts.has_value() || on_dev(*wts, dev, torch::kDouble, R),
              "weights must be contiguous [R] float64");
  TORCH_CHECK(on_dev(pieces, dev, torch::kInt) && pieces.dim() == 2 &&
              pieces.size(0) >= 1 && pieces.size(0) <= 65535 &&
              pieces.size(1) == 4,
              "pieces must be contiguous [E, 4] int32, E <= 65535");
  TORCH_CHECK(Mt * N < (int64_t(1) << 27), "too many parameters");
  check_aligned16({&cohs, &J, &pieces}, "cohs, J and pieces");
  LeverageArgs a = {};
  a.cohs = ccptr(cohs); a.J = ccptr(J); a.Hinv = dp(Hinv);
  a.wts = wts.has_value() ? dp(*wts) : nullptr;
  a.pairs = ip(pairs); a.pieces = ip(pieces);
  a.M = (int)M; a.T = (int)chunk_tab.size(1); a.Nbase = (int)pairs.size(0);
  a.N = (int)N; a.Mt = (int)Mt; a.E = (int)pieces.size(0);
  auto lev = torch::empty({M, R}, torch::dtype(torch::kDouble).device(dev));
  CHECK_HIP(launch_leverage(a, lev.data_ptr<double>(), cur_stream()));
  return lev;
}

// The float64 normal matrices of every chunk (normal_f64.hip): cohs
// [M, R, 4] and J [Mt, N, 4] complex64, optional wts [R] float32, chunk_tab
// [M, T] and pairs [Nbase, 2] int32 with R == T * Nbase; pieces [E, 4] and
// piece_off [Mt + 1] int32 from hip_host._lbfgs_extents, pidx [N, N] int32
// from hip_host._normal_pair_index, sta_off [N + 1] and sta_ent int32 from
// hip_host._lbfgs_stations. Returns JtJ [Mt, 8N, 8N] float64. The caller
// guarantees chunk ids below Mt, pair entries below N and tables built from
// these pairs and this chunk_tab.
torch::Tensor normal_matrices(
    torch::Tensor cohs, torch::Tensor J, c10::optional<torch::Tensor> wts,
    torch::Tensor chunk_tab, torch::Tensor pairs, torch::Tensor pieces,
    torch::Tensor piece_off, torch::Tensor pidx, torch::Tensor sta_off,
    torch::Tensor sta_ent) {
  const torch::Device dev = cohs.device();
  TORCH_CHECK(on_dev(cohs, dev, torch::kComplexFloat) && cohs.dim() == 3 &&
              cohs.size(0) >= 1 && cohs.size(1) >= 1 && cohs.size(2) == 4,
              "cohs must be contiguous [M, R, 4] complex64 on the device");
  const int64_t M = cohs.size(0), R = cohs.size(1);
  check_solution_tables(J, chunk_tab, pairs, M, R, dev);
  const int64_t Mt = J.size(0), N = J.size(1), Nbase = pairs.size(0);
  TORCH_CHECK(!wts.has_value() || on_dev(*wts, dev, torch::kFloat, R),
              "weights must be contiguous [R] float32");
  TORCH_CHECK(on_dev(pieces, dev, torch::kInt) && pieces.dim() == 2 &&
              pieces.size(0) >= 1 && pieces.size(0) <= 65535 &&
              pieces.size(1) == 4,
              "pieces must be contiguous [E, 4] int32, E <= 65535");
  TORCH_CHECK(Mt <= 65535 && N <= 8192, "at most 65535 chunks, 8192 stations");
  TORCH_CHECK(on_dev(piece_off, dev, torch::kInt, Mt + 1) &&
              on_dev(pidx, dev, torch::kInt, N * N) &&
              on_dev(sta_off, dev, torch::kInt, N + 1) &&
              on_dev(sta_ent, dev, torch::kInt) &&
              sta_ent.numel() <= 2 * Nbase,
              "piece_off [Mt + 1], pidx [N, N], sta_off [N + 1] and sta_ent "
              "must be contiguous int32 on the device");
  check_aligned16({&cohs, &J, &pieces}, "cohs, J and pieces");
  NormalF64Args a = {};
  a.cohs = ccptr(cohs); a.J = ccptr(J);
  a.wts = wts.has_value() ? fp(*wts) : nullptr;
  a.pairs = ip(pairs); a.pieces = ip(pieces); a.piece_off = ip(piece_off);
  a.pidx = ip(pidx); a.sta_off = ip(sta_off); a.sta_ent = ip(sta_ent);
  a.M = (int)M; a.T = (int)chunk_tab.size(1); a.Nbase = (int)Nbase;
  a.N = (int)N; a.Mt = (int)Mt; a.E = (int)pieces.size(0);
  const auto f64 = torch::dtype(torch::kDouble).device(dev);
  auto part = torch::empty({pieces.size(0), Nbase, NORMAL_F64_NV}, f64);
  auto JtJ = torch::empty({Mt, 8 * N, 8 * N}, f64);
  CHECK_HIP(launch_normal_f64(a, part.data_ptr<double>(),
                              JtJ.data_ptr<double>(), cur_stream()));
  return JtJ;
}

// Doubles of scratch spd_inverse needs for Mt matrices of n: W [Mt, n, n] and
// the inverted diagonal blocks [Mt, ceil(n / 32), 2, 32, 32].
static int64_t spd_inverse_scratch(int64_t Mt, int64_t n) {
  return Mt * (n * n + (n + 31) / 32 * 2048);
}

// X = (A + mu I)^-1 in float64 (spd_inverse.hip): A [Mt, n, n] float32 or
// float64, read as symmetric from its lower triangle, mu float64 of one
// element or Mt, scratch float64 of spd_inverse_scratch(Mt, n) elements.
// Returns (X [Mt, n, n] float64, info [Mt] int32); a matrix with a
// non-positive pivot has info != 0 and X all NaN.
std::vector<torch::Tensor> spd_inverse(torch::Tensor A, torch::Tensor mu,
                                       torch::Tensor scratch) {
  const torch::Device dev = A.device();
  TORCH_CHECK(A.is_cuda() && A.is_contiguous() &&
              (A.scalar_type() == torch::kFloat ||
               A.scalar_type() == torch::kDouble),
              "A must be a contiguous float32 or float64 device tensor");
  TORCH_CHECK(A.dim() == 3 && A.size(0) >= 1 && A.size(1) == A.size(2),
              "A must be [Mt, n, n] with Mt >= 1");
  const int64_t Mt = A.size(0), n = A.size(1);
  TORCH_CHECK(n >= 8 && n <= SPD_INVERSE_MAXN && n % 8 == 0,
              "n must be a multiple of 8 in 8..", SPD_INVERSE_MAXN, ", got ",
              n);
  TORCH_CHECK(Mt < (int64_t(1) << 20), "too many matrices");
  TORCH_CHECK(on_dev(mu, dev, torch::kDouble) &&
              (mu.numel() == 1 || mu.numel() == Mt),
              "mu must be contiguous float64 on the device, one element or "
              "one per matrix");
  TORCH_CHECK(on_dev(scratch, dev, torch::kDouble) &&
              scratch.numel() >= spd_inverse_scratch(Mt, n),
              "scratch must hold ", spd_inverse_scratch(Mt, n),
              " float64 on the device");
  check_aligned16({&A, &scratch}, "A and scratch");
  auto X = torch::empty({Mt, n, n}, torch::dtype(torch::kDouble).device(dev));
  auto info = torch::zeros({Mt}, torch::dtype(torch::kInt).device(dev));
  SpdInverseArgs a = {};
  a.A = A.data_ptr();
  a.mu = dp(mu);
  a.W = scratch.data_ptr<double>();
  a.D = a.W + Mt * n * n;
  a.info = info.data_ptr<int>();
  a.Mt = (int)Mt; a.n = (int)n;
  a.a_f64 = A.scalar_type() == torch::kDouble;
  a.mu_stride = mu.numel() == 1 ? 0 : 1;
  CHECK_HIP(launch_spd_inverse(a, X.data_ptr<double>(), cur_stream()));
  return {X, info};
}

// The diffuse-cluster coherencies with the spatial model applied
// (diffuse.hip): u, v, w [R] float64 with R == T * Nbase, pairs [Nbase, 2]
// int32, Z [N, Gz*Gz, 2, 2] and Cm [Gc*Gc, 2, 2] complex128, T1 [n1, Gc, Gz]
// and T2 [n2, Gz, n1] float64, n1 = Gc + Gz - 1, n2 = Gz + n1 - 1. Returns
// [R, 2, 2] complex64. The caller guarantees pair entries below N.
torch::Tensor diffuse_coherencies(
    torch::Tensor u, torch::Tensor v, torch::Tensor w, torch::Tensor pairs,
    int64_t T, torch::Tensor Z, torch::Tensor Cm, torch::Tensor T1,
    torch::Tensor T2, double g2, double ll, double mm, double nn1,
    double freq, double fdelta2) {
  const torch::Device dev = u.device();
  TORCH_CHECK(on_dev(pairs, dev, torch::kInt) && pairs.dim() == 2 &&
              pairs.size(0) >= 1 && pairs.size(1) == 2,
              "pairs must be contiguous [Nbase, 2] int32 on the device");
  const int64_t Nbase = pairs.size(0), R = T * Nbase;
  TORCH_CHECK(T >= 1 && T < (int64_t(1) << 31) &&
              Nbase < (int64_t(1) << 31), "rows out of range");
  for (const torch::Tensor* t : {&u, &v, &w})
    TORCH_CHECK(on_dev(*t, dev, torch::kDouble, R) && t->dim() == 1,
                "u, v, w must be contiguous [T * Nbase] float64 on the "
                "device");
  TORCH_CHECK(on_dev(T1, dev, torch::kDouble) && T1.dim() == 3 &&
              on_dev(T2, dev, torch::kDouble) && T2.dim() == 3,
              "T1 and T2 must be contiguous 3-D float64 on the device");
  const int64_t n1 = T1.size(0), Gc = T1.size(1), Gz = T1.size(2);
  const int64_t n2 = T2.size(0);
  TORCH_CHECK(Gc >= 1 && Gz >= 1 && n1 == Gc + Gz - 1 && n2 == Gz + n1 - 1 &&
              T2.size(1) == Gz && T2.size(2) == n1,
              "T1 must be [n1, Gc, Gz] and T2 [n2, Gz, n1]");
  TORCH_CHECK(Gz <= DIFFUSE_MAX_GZ && n2 <= DIFFUSE_MAX_N2,
              "the diffuse kernels take Gz <= ", DIFFUSE_MAX_GZ,
              " and n2 <= ", DIFFUSE_MAX_N2, ", got ", Gz, " and ", n2);
  TORCH_CHECK(on_dev(Z, dev, torch::kComplexDouble) && Z.dim() == 4 &&
              Z.size(0) >= 1 && Z.size(0) <= 65535 &&
              Z.size(1) == Gz * Gz && Z.size(2) == 2 && Z.size(3) == 2,
              "Z must be contiguous [N, Gz*Gz, 2, 2] complex128, N <= 65535");
  TORCH_CHECK(on_dev(Cm, dev, torch::kComplexDouble, Gc * Gc * 4) &&
              Cm.dim() == 3, "Cm must be contiguous [Gc*Gc, 2, 2] complex128");
  const int64_t N = Z.size(0);
  const int64_t RA = DIFFUSE_PAD16(2 * n2), RB = DIFFUSE_PAD16(4 * n2),
                Kp = DIFFUSE_PAD16(4 * n1 * Gz);
  auto scratch = torch::empty({N * (RA + RB) * Kp},
                              torch::dtype(torch::kDouble).device(dev));
  auto out = torch::empty({R, 2, 2},
                          torch::dtype(torch::kComplexFloat).device(dev));
  check_aligned16({&Z, &Cm, &scratch, &out}, "Z, Cm, scratch and out");
  DiffuseArgs a = {};
  a.u = dp(u); a.v = dp(v); a.w = dp(w); a.pairs = ip(pairs);
  a.Z = reinterpret_cast<const double2*>(Z.data_ptr());
  a.C = reinterpret_cast<const double2*>(Cm.data_ptr());
  a.T1 = dp(T1); a.T2 = dp(T2);
  a.A = scratch.data_ptr<double>();
  a.B = a.A + N * RA * Kp;
  a.T = (int)T; a.Nbase = (int)Nbase; a.N = (int)N;
  a.Gz = (int)Gz; a.Gc = (int)Gc;
  a.g2 = g2; a.ll = ll; a.mm = mm; a.nn1 = nn1;
  a.freq = freq; a.fdelta2 = fdelta2;
  CHECK_HIP(launch_diffuse(a, cptr(out), cur_stream()));
  return out;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("jtr_grad", &jtr_grad, "gradient-only accumulation (gfx950)");
  m.attr("DIFFUSE_MAX_GZ") = DIFFUSE_MAX_GZ;
  m.attr("DIFFUSE_MAX_N2") = DIFFUSE_MAX_N2;
  m.def("diffuse_coherencies", &diffuse_coherencies,
        "diffuse-cluster predict with the spatial model (gfx950)",
        py::arg("u"), py::arg("v"), py::arg("w"), py::arg("pairs"),
        py::arg("T"), py::arg("Z"), py::arg("Cm"), py::arg("T1"),
        py::arg("T2"), py::arg("g2"), py::arg("ll"), py::arg("mm"),
        py::arg("nn1"), py::arg("freq"), py::arg("fdelta2"));
  m.attr("SPD_INVERSE_MAXN") = SPD_INVERSE_MAXN;
  m.def("spd_inverse_scratch", &spd_inverse_scratch,
        "float64 elements of scratch spd_inverse needs", py::arg("Mt"),
        py::arg("n"));
  m.def("spd_inverse", &spd_inverse,
        "float64 inverse of damped SPD matrices (gfx950)", py::arg("A"),
        py::arg("mu"), py::arg("scratch"));
  m.def("leverage_rows", &leverage_rows,
        "influence-map leverage, all clusters in one launch (gfx950)",
        py::arg("cohs"), py::arg("J"), py::arg("Hinv"), py::arg("wts"),
        py::arg("chunk_tab"), py::arg("pairs"), py::arg("pieces"));
  m.def("normal_matrices", &normal_matrices,
        "float64 normal matrices of every chunk, two launches (gfx950)",
        py::arg("cohs"), py::arg("J"), py::arg("wts"), py::arg("chunk_tab"),
        py::arg("pairs"), py::arg("pieces"), py::arg("piece_off"),
        py::arg("pidx"), py::arg("sta_off"), py::arg("sta_ent"));
  m.def("rtr_tcg", &rtr_tcg, "RTR truncated-CG inner solve (gfx950)",
        py::arg("JtJ"), py::arg("Jtr"), py::arg("J"), py::arg("iw"),
        py::arg("delta"), py::arg("maxit"), py::arg("kappa"));
  m.attr("JOINT_JTJ_TT") = JOINT_JTJ_TT;
  m.def("joint_jtj", &joint_jtj,
        "joint cross-cluster normal equations (gfx950)", py::arg("x"),
        py::arg("cohs"), py::arg("J"), py::arg("wts"), py::arg("pairs"),
        py::arg("chunk_tab"), py::arg("pieces"), py::arg("etab"),
        py::arg("gtab"), py::arg("cbin"), py::arg("sdst"), py::arg("gdst"),
        py::arg("cpos"), py::arg("sta_off"), py::arg("sta_ent"),
        py::arg("nblk"), py::arg("nbin"), py::arg("cost_only") = false);
  m.def("lbfgs_cost_grad_channels", &lbfgs_cost_grad_channels,
        "multi-channel LBFGS cost and gradient (gfx950)", py::arg("xs"),
        py::arg("cohs"), py::arg("J"), py::arg("chunk_tab"), py::arg("pairs"),
        py::arg("ext"), py::arg("ext_off"), py::arg("sta_off"),
        py::arg("sta_ent"), py::arg("robust_nu") = 0.0);
  m.def("chol_solve", &chol_solve, "batched damped Cholesky solve (gfx950)");
  m.def("chol_solve_mw", &chol_solve_mw,
        "multi-workgroup damped Cholesky solve (gfx950)");
  m.def("chol_solve_blocked", &chol_solve_blocked,
        "blocked damped Cholesky solve, 32 <= n <= 16384 (gfx950)");
  // The predict entry points take the per-source arrays as the record `src`
  // (hip_host.GPUPack.record) or the shapelet mode table as the record
  // `tab` (hip_host.ShapeletTable.record), dicts from field name to tensor.
  m.def("predict_coh", &predict_coh, "coherency predict (gfx950)",
        py::arg("u"), py::arg("v"), py::arg("w"), py::arg("src"),
        py::arg("flux"), py::arg("r1"), py::arg("freq"), py::arg("fdelta2"),
        py::arg("tdelta"), py::arg("beam") = py::none(),
        py::arg("pairs") = py::none(), py::arg("Nbase") = 0,
        py::arg("ejones") = py::none(), py::arg("Nsta") = 0);
  m.def("shapelet_coh_add", &shapelet_coh_add,
        "add shapelet-source coherencies into out (gfx950)",
        py::arg("out"), py::arg("u"), py::arg("v"), py::arg("w"),
        py::arg("tab"), py::arg("flux"), py::arg("r1"), py::arg("freq"),
        py::arg("fdelta2"), py::arg("tdelta"), py::arg("beam") = py::none(),
        py::arg("pairs") = py::none(), py::arg("Nbase") = 0,
        py::arg("ejones") = py::none(), py::arg("Nsta") = 0);
  m.def("predict_coh_channels", &predict_coh_channels,
        "coherency predict, all channels in one launch (gfx950)",
        py::arg("u"), py::arg("v"), py::arg("w"), py::arg("src"),
        py::arg("flux"), py::arg("r1"), py::arg("freqs"), py::arg("fdelta2"),
        py::arg("tdelta"), py::arg("mean") = false,
        py::arg("beam") = py::none(), py::arg("ejones") = py::none(),
        py::arg("pairs") = py::none(), py::arg("Nbase") = 0,
        py::arg("Nsta") = 0);
  m.def("residuals_multifreq", &residuals_multifreq,
        "predict and subtract, all channels in one launch (gfx950)",
        py::arg("x"), py::arg("u"), py::arg("v"), py::arg("w"),
        py::arg("src"), py::arg("flux"), py::arg("r1"), py::arg("freqs"),
        py::arg("fdelta2"), py::arg("tdelta"), py::arg("J"),
        py::arg("chunk_tab"), py::arg("pairs"),
        py::arg("skip") = py::none(), py::arg("beam") = py::none(),
        py::arg("ejones") = py::none(), py::arg("Nsta") = 0);
  m.attr("PREDICT_MF_NF") = PREDICT_MF_NF;
  m.attr("PREDICT_MF_NF_EJ") = PREDICT_MF_NF_EJ;
  m.def("shapelet_coh_channels_add", &shapelet_coh_channels_add,
        "add shapelet-source coherencies of all channels into out (gfx950)",
        py::arg("out"), py::arg("u"), py::arg("v"), py::arg("w"),
        py::arg("tab"), py::arg("flux"), py::arg("r1"), py::arg("freqs"),
        py::arg("fdelta2"), py::arg("tdelta"), py::arg("mean"), py::arg("K"),
        py::arg("beam") = py::none(), py::arg("ejones") = py::none(),
        py::arg("pairs") = py::none(), py::arg("Nbase") = 0,
        py::arg("Nsta") = 0);
  m.def("shapelet_residuals_add", &shapelet_residuals_add,
        "subtract the shapelet-source model of all channels from out "
        "(gfx950)",
        py::arg("out"), py::arg("u"), py::arg("v"), py::arg("w"),
        py::arg("tab"), py::arg("flux"), py::arg("r1"), py::arg("freqs"),
        py::arg("fdelta2"), py::arg("tdelta"), py::arg("J"),
        py::arg("chunk_tab"), py::arg("pairs"), py::arg("skip"), py::arg("K"),
        py::arg("beam") = py::none(), py::arg("ejones") = py::none(),
        py::arg("Nsta") = 0);
  m.attr("SHAPELET_MF_NF") = SHAPELET_MF_NF;
  m.attr("SHAPELET_MF_NF_EJ") = SHAPELET_MF_NF_EJ;
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
