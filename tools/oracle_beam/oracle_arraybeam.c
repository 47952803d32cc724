/* Oracle driver: evaluate the REFERENCE station beam gains (arraybeam,
 * stationbeam.c:49) for one array, single-stage (STAT_SINGLE over the tile
 * centroids) and two-stage (STAT_TILE), with wideband=1 (beamformer
 * frequency = evaluation frequency), so beams.array_beam_gains and
 * beams.station_beam_gains can be checked value by value.
 *
 * stdin (whitespace separated, reference conventions: x,y,z metres with
 * (x,y,z) = (N,-E,U); angles rad; times JD days; ra0,dec0 the station
 * pointing, b_ra0,b_dec0 the tile pointing):
 *   N K T F
 *   lon lat ra0 dec0 b_ra0 b_dec0
 *   T times, F frequencies, K lines "ra dec"
 *   per station: ntiles, then 16 dipole "x y z", then ntiles centroid lines
 * stdout: for bf in (single, tile), t, f, k: one line of N gains. */
#include <stdio.h>
#include <stdlib.h>
#include <Dirac.h>
#include <Dirac_radio.h>

static double rd(void) {
  double v;
  if (scanf("%lf", &v) != 1) { fprintf(stderr, "short input\n"); exit(1); }
  return v;
}

int main(void) {
  int N = (int)rd(), K = (int)rd(), T = (int)rd(), F = (int)rd();
  double lon = rd(), lat = rd(), ra0 = rd(), dec0 = rd();
  double b_ra0 = rd(), b_dec0 = rd();
  double *tm = calloc(T, sizeof(double)), *fq = calloc(F, sizeof(double));
  double *ra = calloc(K, sizeof(double)), *dec = calloc(K, sizeof(double));
  for (int i = 0; i < T; i++) tm[i] = rd();
  for (int i = 0; i < F; i++) fq[i] = rd();
  for (int i = 0; i < K; i++) { ra[i] = rd(); dec[i] = rd(); }
  double *lons = calloc(N, sizeof(double)), *lats = calloc(N, sizeof(double));
  int *Nelem = calloc(N, sizeof(int));
  /* STAT_TILE layout: 16 dipoles first, centroids after; the single-stage
     call gets pointers to the centroids alone */
  double **x = calloc(N, sizeof(double *)), **y = calloc(N, sizeof(double *));
  double **z = calloc(N, sizeof(double *));
  double **cx = calloc(N, sizeof(double *)), **cy = calloc(N, sizeof(double *));
  double **cz = calloc(N, sizeof(double *));
  for (int n = 0; n < N; n++) {
    lons[n] = lon; lats[n] = lat;
    Nelem[n] = (int)rd();
    int tot = Nelem[n] + HBA_TILE_SIZE;
    x[n] = calloc(tot, sizeof(double));
    y[n] = calloc(tot, sizeof(double));
    z[n] = calloc(tot, sizeof(double));
    for (int e = 0; e < tot; e++) { x[n][e] = rd(); y[n][e] = rd();
                                    z[n][e] = rd(); }
    cx[n] = x[n] + HBA_TILE_SIZE;
    cy[n] = y[n] + HBA_TILE_SIZE;
    cz[n] = z[n] + HBA_TILE_SIZE;
  }
  double *g = calloc(N, sizeof(double));
  for (int bf = 0; bf < 2; bf++)
    for (int t = 0; t < T; t++)
      for (int f = 0; f < F; f++)
        for (int k = 0; k < K; k++) {
          if (bf == 0)
            arraybeam(ra[k], dec[k], STAT_SINGLE, b_ra0, b_dec0, ra0, dec0,
                      fq[f], fq[f], N, lons, lats, tm[t], Nelem, cx, cy, cz,
                      g, 1);
          else
            arraybeam(ra[k], dec[k], STAT_TILE, b_ra0, b_dec0, ra0, dec0,
                      fq[f], fq[f], N, lons, lats, tm[t], Nelem, x, y, z,
                      g, 1);
          for (int n = 0; n < N; n++)
            printf("%.17g%c", g[n], n + 1 < N ? ' ' : '\n');
        }
  return 0;
}
