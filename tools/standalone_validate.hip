// Torch-free standalone validator for two kernel paths, done in about a
// minute (no python/torch startup). It calls the launchers through the
// argument structs of launchers.h, as bindings.cpp does:
//   1. k_cholmw_panel_big — chunked-panel Cholesky at n=4096
//      (and n=512 through the same harness as a control)
//   2. k_predict_coh beam argument — all-ones beam must reproduce the
//      no-beam output exactly; a scalar beam must scale a single-source
//      cluster's output by bg[p]*bg[q] row-wise.
// Build (cross-compile, no GPU needed):
//   hipcc --offload-arch=gfx950 -O2 -o tools/standalone_validate \
//       tools/standalone_validate.hip
// Run on the box: ./tools/standalone_validate   (prints PASS/FAIL)
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>
#include "../sagecal_amd/ops/hip/launchers.hip"

#define CHK(x) do { hipError_t e = (x); if (e != hipSuccess) { \
  printf("FAIL hip %s at %d\n", hipGetErrorString(e), __LINE__); \
  exit(1); } } while (0)

static unsigned lcg_state = 12345u;
static float frand() {
  lcg_state = lcg_state * 1664525u + 1013904223u;
  return ((lcg_state >> 9) & 0x3fffff) / (float)0x400000 - 0.5f;
}

static int test_chol(int n) {
  const int batch = 1;
  std::vector<float> A((size_t)n * n), b(n);
  // symmetric diagonally-dominant SPD
  for (int i = 0; i < n; i++)
    for (int j = 0; j <= i; j++) {
      float v = frand();
      A[(size_t)i * n + j] = v;
      A[(size_t)j * n + i] = v;
    }
  for (int i = 0; i < n; i++) {
    double rs = 0;
    for (int j = 0; j < n; j++) if (j != i) rs += fabs(A[(size_t)i * n + j]);
    A[(size_t)i * n + i] = (float)(rs + 1.0);
    b[i] = frand();
  }
  float mu_h = 0.5f;
  float *dA, *db, *dmu, *dL, *dx;
  int *dinfo;
  CHK(hipMalloc(&dA, sizeof(float) * n * n));
  CHK(hipMalloc(&db, sizeof(float) * n));
  CHK(hipMalloc(&dmu, sizeof(float)));
  CHK(hipMalloc(&dL, sizeof(float) * 2 * (size_t)n * n));
  CHK(hipMalloc(&dx, sizeof(float) * n));
  CHK(hipMalloc(&dinfo, sizeof(int)));
  CHK(hipMemcpy(dA, A.data(), sizeof(float) * n * n,
                hipMemcpyHostToDevice));
  CHK(hipMemcpy(db, b.data(), sizeof(float) * n, hipMemcpyHostToDevice));
  CHK(hipMemcpy(dmu, &mu_h, sizeof(float), hipMemcpyHostToDevice));
  CHK(hipMemset(dinfo, 0, sizeof(int)));
  CHK(launch_chol_mw(dA, db, dmu, n, batch, dL, dx, dinfo, 0));
  CHK(hipDeviceSynchronize());
  std::vector<float> x(n);
  int info_h = 0;
  CHK(hipMemcpy(x.data(), dx, sizeof(float) * n, hipMemcpyDeviceToHost));
  CHK(hipMemcpy(&info_h, dinfo, sizeof(int), hipMemcpyDeviceToHost));
  // residual (A + mu I) x - b
  double rmax = 0, bmax = 0;
  for (int i = 0; i < n; i++) {
    double s = mu_h * (double)x[i];
    for (int j = 0; j < n; j++) s += (double)A[(size_t)i * n + j] * x[j];
    rmax = fmax(rmax, fabs(s - b[i]));
    bmax = fmax(bmax, fabs((double)b[i]));
  }
  hipFree(dA); hipFree(db); hipFree(dmu); hipFree(dL); hipFree(dx);
  hipFree(dinfo);
  double rel = rmax / fmax(bmax, 1e-30);
  printf("chol n=%d: info=%d rel_resid=%.3e -> %s\n", n, info_h, rel,
         (info_h == 0 && rel < 1e-2) ? "PASS" : "FAIL");
  return (info_h == 0 && rel < 1e-2) ? 0 : 1;
}

static int test_beam_predict() {
  // 2 clusters x 1 point source each, N=8 stations, T=2 slots
  const int N = 8, T = 2, K = 2, M = 2, Nbase = N * (N - 1) / 2;
  const int R = Nbase * T;
  std::vector<double> u(R), v(R), w(R), ll(K), mm(K), nn1(K);
  std::vector<float> sI(K), sQ(K), sU(K), sV(K), eX(K, 0), eY(K, 0),
      eP(K, 0), cxi(K, 1), sxi(K, 0), cphi(K, 1), sphi(K, 0), r1(K, 0);
  std::vector<int> stype(K, 0), coff = {0, 1, 2};
  std::vector<int> pairs;
  for (int p = 0; p < N; p++)
    for (int q = p + 1; q < N; q++) { pairs.push_back(p);
                                      pairs.push_back(q); }
  for (int r = 0; r < R; r++) { u[r] = frand() * 1e-5;
                                v[r] = frand() * 1e-5;
                                w[r] = frand() * 1e-6; }
  for (int k = 0; k < K; k++) { ll[k] = 0.01 * (k + 1);
                                mm[k] = -0.02 * (k + 1);
                                nn1[k] = -1e-4 * (k + 1);
                                sI[k] = 1.0f + k; sQ[k] = 0.1f;
                                sU[k] = 0.05f; sV[k] = 0.02f; }
  std::vector<float> beam1((size_t)T * K * N, 1.0f);      // all ones
  std::vector<float> beam2((size_t)T * K * N);
  for (size_t i = 0; i < beam2.size(); i++) beam2[i] = 0.5f + 0.25f *
      (float)((i * 37) % 7);
  double freq = 150e6, fdelta2 = 5e3, tdelta = 0.0;

  auto up = [&](auto& h, auto*& d) {
    CHK(hipMalloc(&d, h.size() * sizeof(h[0])));
    CHK(hipMemcpy(d, h.data(), h.size() * sizeof(h[0]),
                  hipMemcpyHostToDevice));
  };
  double *du, *dv, *dw, *dll, *dmm, *dnn;
  float *dsI, *dsQ, *dsU, *dsV, *deX, *deY, *deP, *dcxi, *dsxi, *dcphi,
      *dsphi, *dr1, *dbeam1, *dbeam2;
  int *dstype, *dcoff, *dpairs;
  up(u, du); up(v, dv); up(w, dw); up(ll, dll); up(mm, dmm);
  up(nn1, dnn); up(sI, dsI); up(sQ, dsQ); up(sU, dsU); up(sV, dsV);
  up(eX, deX); up(eY, deY); up(eP, deP); up(cxi, dcxi); up(sxi, dsxi);
  up(cphi, dcphi); up(sphi, dsphi); up(r1, dr1); up(stype, dstype);
  up(coff, dcoff); up(pairs, dpairs); up(beam1, dbeam1); up(beam2, dbeam2);
  float2 *o0, *o1, *o2;
  CHK(hipMalloc(&o0, sizeof(float2) * M * R * 4));
  CHK(hipMalloc(&o1, sizeof(float2) * M * R * 4));
  CHK(hipMalloc(&o2, sizeof(float2) * M * R * 4));
  RowsUVW rows = {};
  rows.u = du; rows.v = dv; rows.w = dw; rows.R = R;
  SourceArrays src = {};
  src.ll = dll; src.mm = dmm; src.nn1 = dnn;
  src.sI = dsI; src.sQ = dsQ; src.sU = dsU; src.sV = dsV;
  src.eX = deX; src.eY = deY; src.eP = deP;
  src.cxi = dcxi; src.sxi = dsxi; src.cphi = dcphi; src.sphi = dsphi;
  src.r1 = dr1; src.stype = dstype; src.cluster_off = dcoff; src.M = M;
  const Channel ch = {freq, fdelta2, tdelta};
  BeamArgs nobeam = {}, bm1 = {}, bm2 = {};
  bm1.beam = dbeam1; bm1.pairs = dpairs;
  bm1.Nbase = Nbase; bm1.Ktot = K; bm1.Nsta = N;
  bm2 = bm1;
  bm2.beam = dbeam2;
  CHK(launch_predict_coh(rows, src, ch, nobeam, o0, 0));
  CHK(launch_predict_coh(rows, src, ch, bm1, o1, 0));
  CHK(launch_predict_coh(rows, src, ch, bm2, o2, 0));
  CHK(hipDeviceSynchronize());
  std::vector<float2> h0(M * R * 4), h1(M * R * 4), h2(M * R * 4);
  CHK(hipMemcpy(h0.data(), o0, sizeof(float2) * h0.size(),
                hipMemcpyDeviceToHost));
  CHK(hipMemcpy(h1.data(), o1, sizeof(float2) * h1.size(),
                hipMemcpyDeviceToHost));
  CHK(hipMemcpy(h2.data(), o2, sizeof(float2) * h2.size(),
                hipMemcpyDeviceToHost));
  // all-ones beam == no beam, bitwise
  int fail = 0;
  for (size_t i = 0; i < h0.size(); i++)
    if (h0[i].x != h1[i].x || h0[i].y != h1[i].y) { fail = 1; break; }
  printf("beam all-ones == no-beam: %s\n", fail ? "FAIL" : "PASS");
  // scalar relation per (cluster ci, row r): out2 = s * out0 with
  // s = bg[t, ci, p] * bg[t, ci, q]  (cluster ci has exactly source ci)
  double emax = 0, ref = 0;
  for (int ci = 0; ci < M; ci++)
    for (int r = 0; r < R; r++) {
      int t = r / Nbase, bl = r % Nbase;
      int p = pairs[2 * bl], q = pairs[2 * bl + 1];
      float s = beam2[((size_t)t * K + ci) * N + p] *
                beam2[((size_t)t * K + ci) * N + q];
      for (int i = 0; i < 4; i++) {
        float2 a = h0[((size_t)ci * R + r) * 4 + i];
        float2 b2 = h2[((size_t)ci * R + r) * 4 + i];
        emax = fmax(emax, fabs((double)b2.x - s * a.x));
        emax = fmax(emax, fabs((double)b2.y - s * a.y));
        ref = fmax(ref, fabs((double)b2.x));
      }
    }
  double rel = emax / fmax(ref, 1e-30);
  printf("beam scalar relation rel err %.3e -> %s\n", rel,
         rel < 1e-5 ? "PASS" : "FAIL");
  return fail || (rel >= 1e-5);
}

static int test_chol_graph(int n) {
  // hipGraph-capture the launch_chol_mw sequence (what the production
  // LM graph path replays) and verify the replayed solve
  const int batch = 2;
  std::vector<float> A((size_t)n * n), b((size_t)batch * n);
  for (int i = 0; i < n; i++)
    for (int j = 0; j <= i; j++) {
      float v = frand();
      A[(size_t)i * n + j] = v;
      A[(size_t)j * n + i] = v;
    }
  for (int i = 0; i < n; i++) {
    double rs = 0;
    for (int j = 0; j < n; j++) if (j != i) rs += fabs(A[(size_t)i*n+j]);
    A[(size_t)i * n + i] = (float)(rs + 1.0);
  }
  for (int i = 0; i < batch * n; i++) b[i] = frand();
  float mu_h[2] = {0.5f, 0.25f};
  float *dA, *db, *dmu, *dL, *dx;
  int *dinfo;
  CHK(hipMalloc(&dA, sizeof(float) * (size_t)batch * n * n));
  CHK(hipMalloc(&db, sizeof(float) * batch * n));
  CHK(hipMalloc(&dmu, sizeof(float) * batch));
  CHK(hipMalloc(&dL, sizeof(float) * 2 * (size_t)batch * n * n));
  CHK(hipMalloc(&dx, sizeof(float) * batch * n));
  CHK(hipMalloc(&dinfo, sizeof(int) * batch));
  for (int bb2 = 0; bb2 < batch; bb2++)
    CHK(hipMemcpy(dA + (size_t)bb2 * n * n, A.data(),
                  sizeof(float) * (size_t)n * n, hipMemcpyHostToDevice));
  CHK(hipMemcpy(db, b.data(), sizeof(float) * batch * n,
                hipMemcpyHostToDevice));
  CHK(hipMemcpy(dmu, mu_h, sizeof(float) * batch,
                hipMemcpyHostToDevice));
  CHK(hipMemset(dinfo, 0, sizeof(int) * batch));
  hipStream_t st;
  CHK(hipStreamCreate(&st));
  hipGraph_t graph;
  hipGraphExec_t gexec;
  CHK(hipStreamBeginCapture(st, hipStreamCaptureModeGlobal));
  CHK(launch_chol_mw(dA, db, dmu, n, batch, dL, dx, dinfo, st));
  CHK(hipStreamEndCapture(st, &graph));
  CHK(hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0));
  CHK(hipGraphLaunch(gexec, st));
  CHK(hipStreamSynchronize(st));
  std::vector<float> x(batch * n);
  int info_h[2];
  CHK(hipMemcpy(x.data(), dx, sizeof(float) * batch * n,
                hipMemcpyDeviceToHost));
  CHK(hipMemcpy(info_h, dinfo, sizeof(int) * batch,
                hipMemcpyDeviceToHost));
  double worst = 0;
  for (int bb2 = 0; bb2 < batch; bb2++) {
    double rmax = 0, bmax = 0;
    for (int i = 0; i < n; i++) {
      double s2 = mu_h[bb2] * (double)x[bb2 * n + i];
      for (int j = 0; j < n; j++)
        s2 += (double)A[(size_t)i * n + j] * x[bb2 * n + j];
      rmax = fmax(rmax, fabs(s2 - b[bb2 * n + i]));
      bmax = fmax(bmax, fabs((double)b[bb2 * n + i]));
    }
    worst = fmax(worst, rmax / fmax(bmax, 1e-30));
  }
  hipFree(dA); hipFree(db); hipFree(dmu); hipFree(dL); hipFree(dx);
  hipFree(dinfo);
  int ok = (info_h[0] == 0 && info_h[1] == 0 && worst < 1e-2);
  printf("chol GRAPH n=%d batch=2: info=%d,%d rel_resid=%.3e -> %s\n",
         n, info_h[0], info_h[1], worst, ok ? "PASS" : "FAIL");
  return !ok;
}

int main() {
  int rc = 0;
  rc |= test_chol(512);      // control: the validated kernel path
  rc |= test_chol(4096);     // chunked-panel path
  rc |= test_chol_graph(4096);  // graph-captured replay, batch 2
  rc |= test_beam_predict(); // fused-beam path
  printf(rc ? "OVERALL FAIL\n" : "OVERALL PASS\n");
  return rc;
}
