"""Host side of the station beam: geometry object, array-factor gains and
the all-(t,k) element E-Jones against the per-timeslot code they replace.
"""
import numpy as np
import pytest
import torch

import shapelet_sky as S
from sagecal_amd import beams, coords

TMJD = np.array([57000.0, 57000.0001, 57000.0002])
LON, LAT = 0.1, 0.92


def _cfg(counts, seed=7, lat=LAT):
    rng = np.random.default_rng(seed)
    elems = [rng.uniform(-30, 30, (c, 3)) for c in counts]
    return beams.ArrayConfig(elems, LON, lat, 0.0, S.DEC0)


@pytest.fixture(scope='module')
def sky():
    pack, _ = S.make_pack()
    ra, dec = beams._pack_radec(pack, S.DEC0)
    u, v, w, bb, Nbase = S.uvw_rows()
    return dict(pack=pack, ra=ra, dec=dec, uvw=(u, v, w), bb=bb,
                Nbase=Nbase)


@pytest.mark.parametrize('counts', [(16,) * 10, (1, 5, 16, 65)],
                         ids=['equal', 'jagged'])
def test_gains_match_array_beam(sky, counts):
    cfg = _cfg(counts)
    geom = beams.beam_geometry(cfg, sky['ra'], sky['dec'], TMJD)
    assert geom.du.shape == (3, 9, 3) and geom.below.shape == (3, 9)
    assert geom.az.shape == (3, 9) and geom.el.shape == (3, 9)
    got = beams.array_beam_gains(cfg, geom, S.FREQ0, 'cpu')
    ref = beams.array_beam(cfg, sky['ra'], sky['dec'], [S.FREQ0], TMJD)
    ref = ref[..., 0].abs().permute(2, 1, 0)
    assert got.shape == (3, 9, len(counts)) and got.dtype == torch.float64
    err = float(((got - ref).abs() / ref.abs()).max())
    print('array_beam_gains vs array_beam, max rel err:', err)
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=0.0)


def test_gain_edge_values(sky):
    cfg = _cfg((1, 5, 16, 65))
    # the 9 sources, the pointing direction, and its antipode
    ra = np.concatenate([sky['ra'], [cfg.b_ra0, cfg.b_ra0 + np.pi]])
    dec = np.concatenate([sky['dec'], [cfg.b_dec0, -cfg.b_dec0]])
    geom = beams.beam_geometry(cfg, ra, dec, TMJD)
    g = beams.array_beam_gains(cfg, geom, S.FREQ0, 'cpu')
    assert not geom.below[:, :10].any() and geom.below[:, 10].all()
    # one-element station: exactly 1 above the horizon
    assert bool((g[:, :10, 0] == 1.0).all())
    # pointing direction: every phasor is 1
    assert float((g[:, 9, :] - 1.0).abs().max()) <= 1e-12
    # antipode of the pointing is below the horizon: exactly 0
    assert bool((g[:, 10, :] == 0.0).all())


def _loop_jones(coeffs, cfg, ra, dec, freq):
    """The per-timeslot loop of predict_coh_withbeam: [K, T, 2, 2]."""
    gmst = coords.jd_to_gmst(TMJD + 2400000.5)
    Es = []
    for g in np.atleast_1d(gmst):
        _, az, el = beams._direction_enu(ra, dec, cfg.lon, cfg.lat, g)
        E = beams.element_beam(coeffs, az, np.maximum(el, 0.0), freq)
        E[torch.from_numpy(el < 0)] = 0
        Es.append(E)
    return torch.stack(Es, dim=1)


@pytest.mark.parametrize('kind', ['synthetic', 'lba'])
def test_element_jones_matches_timeslot_loop(sky, kind):
    cfg = _cfg((16,) * 10)
    coeffs = (beams.make_synthetic_element_coeffs(freqs=(S.FREQ0,))
              if kind == 'synthetic' else beams.LofarElementCoeffs.load(kind))
    # one source below the horizon so the zeroing is compared too
    ra = np.concatenate([sky['ra'], [cfg.b_ra0 + np.pi]])
    dec = np.concatenate([sky['dec'], [-cfg.b_dec0]])
    geom = beams.beam_geometry(cfg, ra, dec, TMJD)
    got = beams.element_jones(coeffs, geom, S.FREQ0)
    ref = _loop_jones(coeffs, cfg, ra, dec, S.FREQ0).permute(1, 0, 2, 3)
    assert got.shape == (3, 10, 2, 2) and got.dtype == torch.complex128
    assert float(ref[:, :9].abs().min()) > 0 and not ref[:, 9].any()
    assert torch.equal(got, ref)


@pytest.mark.parametrize('mode', [1, 2, 3])
def test_geom_argument_changes_nothing(sky, mode):
    cfg = _cfg((16,) * 10)
    args = (sky['pack'], *sky['uvw'], S.FREQ0, S.FREQ0, S.FDELTA, S.TDELTA,
            S.DEC0, cfg, TMJD, sky['bb'], sky['Nbase'], 3)
    ref = beams.predict_coh_withbeam(*args, mode=mode)
    geom = beams.beam_geometry(cfg, sky['ra'], sky['dec'], TMJD)
    got = beams.predict_coh_withbeam(*args, mode=mode, geom=geom)
    assert float(ref.abs().max()) > 0
    assert torch.equal(got, ref)
