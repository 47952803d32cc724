"""Record tests/golden/reference_arraybeam.json from the reference's own
arraybeam (stationbeam.c:49), STAT_SINGLE and STAT_TILE.

  REF=<reference tree> python tools/oracle_beam/record_arraybeam.py

builds oracle_arraybeam (build_oracle_beam.sh, into oracle/_ref/beam, which
git ignores), feeds it the seeded inputs below and stores inputs and gains
together. The fixture keeps OUR conventions: ENU offsets in metres, times in
MJD days, `b_ra0, b_dec0` the station pointing and `tile_ra0, tile_dec0` the
tile pointing. The driver gets the reference's: (x, y, z) = (N, -E, U), JD,
`ra0, dec0` = our station pointing, `b_ra0, b_dec0` = our tile pointing, the
16 dipoles of a station first and its tile centroids after, Nelem counting
tiles only, every station at the same longitude and latitude, wideband=1.
"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TILES = (1, 3, 24, 48, 130, 17)
D = 16


def make_inputs(seed=20):
    rng = np.random.default_rng(seed)
    b_ra0, b_dec0 = 0.0, np.pi / 4
    inp = dict(
        lon=0.1, lat=0.92, b_ra0=b_ra0, b_dec0=b_dec0,
        tile_ra0=b_ra0 + 0.02, tile_dec0=b_dec0 - 0.014,
        tmjd=[57000.0, 57000.01], freqs=[120e6, 150e6, 180e6])
    # 7 sources around the pointing and its antipode, below the horizon
    ra = b_ra0 + rng.uniform(-0.4, 0.4, 7)
    dec = b_dec0 + rng.uniform(-0.3, 0.3, 7)
    inp['ra'] = np.concatenate([ra, [b_ra0 + np.pi]]).tolist()
    inp['dec'] = np.concatenate([dec, [-b_dec0]]).tolist()
    cent, dip = [], []
    grid = (np.arange(4) - 1.5) * 1.25
    gx, gy = np.meshgrid(grid, grid)
    for nt in TILES:
        c = np.column_stack([rng.uniform(-30, 30, nt),
                             rng.uniform(-30, 30, nt),
                             rng.uniform(-0.5, 0.5, nt)])
        cent.append(np.round(c, 4).tolist())
        # 4x4 dipole grid, rotated per station, slightly perturbed
        a = rng.uniform(0, np.pi)
        e = np.cos(a) * gx.ravel() - np.sin(a) * gy.ravel()
        n = np.sin(a) * gx.ravel() + np.cos(a) * gy.ravel()
        d = np.column_stack([e, n, np.zeros(D)]) \
            + rng.uniform(-0.05, 0.05, (D, 3))
        dip.append(np.round(d, 4).tolist())
    inp['centroid_enu'] = cent
    inp['dipole_enu'] = dip
    return inp


def driver_text(inp):
    def xyz(enu):
        return ['%.17g %.17g %.17g' % (n, -e, u) for e, n, u in enu]
    K, T, F = len(inp['ra']), len(inp['tmjd']), len(inp['freqs'])
    out = ['%d %d %d %d' % (len(TILES), K, T, F),
           ' '.join('%.17g' % inp[k] for k in (
               'lon', 'lat', 'b_ra0', 'b_dec0', 'tile_ra0', 'tile_dec0')),
           ' '.join('%.17g' % (t + 2400000.5) for t in inp['tmjd']),
           ' '.join('%.17g' % f for f in inp['freqs'])]
    out += ['%.17g %.17g' % rd for rd in zip(inp['ra'], inp['dec'])]
    for c, d in zip(inp['centroid_enu'], inp['dipole_enu']):
        out += [str(len(c))] + xyz(d) + xyz(c)
    return '\n'.join(out) + '\n'


def main():
    outdir = os.path.join(ROOT, 'oracle', '_ref', 'beam')
    subprocess.run(['bash', os.path.join(HERE, 'build_oracle_beam.sh'),
                    outdir], check=True)
    inp = make_inputs()
    res = subprocess.run([os.path.join(outdir, 'oracle_arraybeam')],
                         input=driver_text(inp), capture_output=True,
                         text=True, check=True)
    K, T, F = len(inp['ra']), len(inp['tmjd']), len(inp['freqs'])
    g = np.array([[float(v) for v in line.split()]
                  for line in res.stdout.splitlines()])
    g = g.reshape(2, T, F, K, len(TILES)).transpose(0, 2, 1, 3, 4)
    fix = dict(
        source='arraybeam (stationbeam.c), wideband=1, one lon/lat for '
               'every station; gains are [F, T, K, N]',
        inputs=inp, gains_single=g[0].tolist(), gains_tile=g[1].tolist())
    path = os.path.join(ROOT, 'tests', 'golden', 'reference_arraybeam.json')
    with open(path, 'w') as fh:
        json.dump(fix, fh, indent=0)
        fh.write('\n')
    print('wrote', path, os.path.getsize(path), 'bytes;',
          'max |tile - single| =', float(np.abs(g[1] - g[0]).max()))


if __name__ == '__main__':
    sys.exit(main())
