"""Inputs shared by the two-stage (HBA tile) beam tests, test_tile_beam.py
and test_gpu_tile_beam.py: the recorded reference fixture, the station
layouts of the kernel tests and an fp64 numpy evaluation of the gain
definition that uses none of the library's gain code."""
import json
import os

import numpy as np

from sagecal_amd import beams
from sagecal_amd.constants import C_LIGHT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                      'reference_arraybeam.json')
LON, LAT = 0.1, 0.92
TMJD = np.array([57000.0, 57000.0001, 57000.0002])
# one-tile station, a few tiles, 130 = two LDS passes of 128; 6 stations
# leave the second block of 4 stations half full
TILES = (1, 3, 24, 48, 130, 17)
D = 16


def load_fixture():
    with open(GOLDEN) as fh:
        fx = json.load(fh)
    inp = fx['inputs']
    return (inp, np.array(fx['gains_single']), np.array(fx['gains_tile']))


def fixture_cfg(inp, two):
    return beams.ArrayConfig(
        [np.array(c) for c in inp['centroid_enu']], inp['lon'], inp['lat'],
        inp['b_ra0'], inp['b_dec0'], tile_enu=np.array(inp['dipole_enu']),
        bf_type='tile' if two else 'single', tile_ra0=inp['tile_ra0'],
        tile_dec0=inp['tile_dec0'])


def layouts(nsta_tiles=TILES, seed=41, ndip=D, shared=False):
    """(centroids: list of [c, 3], dipoles: [N, ndip, 3] or [ndip, 3])."""
    rng = np.random.default_rng(seed)
    cent = [rng.uniform(-30, 30, (c, 3)) for c in nsta_tiles]
    dip = rng.uniform(-2.5, 2.5, (len(nsta_tiles), ndip, 3))
    return cent, (dip[0] if shared else dip)


def tile_cfg(cent, dip, b_ra0, b_dec0, dra=0.02, ddec=-0.014,
             bf_type='tile'):
    return beams.ArrayConfig(cent, LON, LAT, b_ra0, b_dec0, tile_enu=dip,
                             bf_type=bf_type, tile_ra0=b_ra0 + dra,
                             tile_dec0=b_dec0 + ddec)


def formula_gains(cent, dip, geom, freqs, two=True):
    """[F, T, K, N] float64 straight from the definition:
    |mean_c exp(i kf c.du)| * |mean_d exp(i kf d.du_tile)|, 0 below."""
    dip = np.asarray(dip)
    out = np.zeros((len(freqs), geom.T, geom.K, len(cent)))
    for fi, f in enumerate(freqs):
        kf = 2.0 * np.pi * f / C_LIGHT
        for n, c in enumerate(cent):
            g = np.abs(np.exp(1j * kf * (geom.du @ np.asarray(c).T))
                       .mean(axis=-1))
            if two:
                d = dip[n] if dip.ndim == 3 else dip
                g = g * np.abs(np.exp(1j * kf * (geom.du_tile @ d.T))
                               .mean(axis=-1))
            out[fi, :, :, n] = np.where(geom.below, 0.0, g)
    return out
