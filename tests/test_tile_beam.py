"""Two-stage HBA tile beamformer on the host: the recorded reference
arraybeam (STAT_SINGLE and STAT_TILE) replayed through the CPU gains, the
factorisation identity, argument checks, predict_coh_withbeam modes 1 and
2 against a hand-built sum, and the command-line wiring."""
import types

import numpy as np
import pytest
import torch

import shapelet_sky as S
import tile_beam_cases as C
from sagecal_amd import beams, msdata, sky as skymod
from sagecal_amd.ops.reference import SourcePack


@pytest.fixture(scope='module')
def fixture():
    return C.load_fixture()


def test_fixture_meets_its_conditions(fixture):
    inp, single, tile = fixture
    assert [len(c) for c in inp['centroid_enu']] == list(C.TILES)
    assert np.array(inp['dipole_enu']).shape == (6, 16, 3)
    assert single.shape == tile.shape == (3, 2, 8, 6)
    sep = np.hypot((inp['tile_ra0'] - inp['b_ra0']) * np.cos(inp['b_dec0']),
                   inp['tile_dec0'] - inp['b_dec0'])
    print('pointing separation (rad):', sep)
    assert 0.01 < sep < 0.04
    diff = float(np.abs(tile - single).max())
    print('max |two-stage - single-stage| in the fixture:', diff)
    assert diff >= 0.1
    # exactly one source below the horizon, 0 for every station
    dark = (tile == 0).all(axis=(0, 1, 3))
    assert dark.tolist() == [False] * 7 + [True]
    assert (single[:, :, 7] == 0).all()
    assert (tile[:, :, :7] > 0).all()


@pytest.mark.parametrize('two', [False, True], ids=['single', 'tile'])
def test_cpu_gains_reproduce_reference_arraybeam(fixture, two):
    """1e-9 absolute: the reference's own GMST and az/el rounding, which
    the oracle tests pin at 1e-9 rad; the formulas agree to ~1e-10."""
    inp, single, tile = fixture
    ref = tile if two else single
    cfg = C.fixture_cfg(inp, two)
    geom = beams.beam_geometry(cfg, inp['ra'], inp['dec'],
                               np.array(inp['tmjd']))
    assert (geom.du_tile is not None) == two
    got = beams.station_beam_gains(cfg, geom, inp['freqs'], 'cpu')
    assert got.shape == ref.shape and got.dtype == torch.float64
    err = float(np.abs(got.numpy() - ref).max())
    print('station_beam_gains vs reference arraybeam, max abs:', err)
    assert err < 1e-9
    for fi, f in enumerate(inp['freqs']):
        one = beams.array_beam_gains(cfg, geom, f, 'cpu')
        err = float(np.abs(one.numpy() - ref[fi]).max())
        print(f'array_beam_gains at {f:.4g} Hz vs reference, max abs:', err)
        assert err < 1e-9
    assert bool((got[:, :, 7] == 0).all())


@pytest.fixture(scope='module')
def sky():
    pack, _ = S.make_pack()
    ra, dec = beams._pack_radec(pack, S.DEC0)
    u, v, w, bb, Nbase = S.uvw_rows()
    return dict(pack=pack, ra=ra, dec=dec, uvw=(u, v, w), bb=bb,
                Nbase=Nbase)


def test_two_stage_factorises(sky):
    """Equal pointings: sum_c sum_d exp(i k (c+d).du) is the product of
    the two sums, so the two-stage gain is the single-stage gain of the
    expanded layout. Stations 0 and 3 have one tile."""
    cent, dip = C.layouts((1, 3, 24, 1, 17))
    cfg = C.tile_cfg(cent, dip, 0.0, S.DEC0, dra=0.0, ddec=0.0)
    full = [(np.asarray(c)[:, None, :] + dip[n][None, :, :]).reshape(-1, 3)
            for n, c in enumerate(cent)]
    cfg1 = beams.ArrayConfig(full, C.LON, C.LAT, 0.0, S.DEC0)
    ra = np.concatenate([sky['ra'], [np.pi]])
    dec = np.concatenate([sky['dec'], [-S.DEC0]])
    geom = beams.beam_geometry(cfg, ra, dec, C.TMJD)
    geom1 = beams.beam_geometry(cfg1, ra, dec, C.TMJD)
    assert np.array_equal(geom.du, geom.du_tile)
    freqs = [120e6, 150e6, 180e6]
    got = beams.station_beam_gains(cfg, geom, freqs, 'cpu')
    ref = beams.station_beam_gains(cfg1, geom1, freqs, 'cpu')
    err = float((got - ref).abs().max())
    print('two-stage vs expanded single-stage, max abs:', err)
    assert err < 1e-12
    assert float(ref[:, :, :9].min()) > 0 and not ref[:, :, 9].any()
    # the one-tile stations are the bare dipole factor
    dipf = C.formula_gains(cent, dip, geom, freqs) \
        / C.formula_gains(cent, dip, geom, freqs, two=False).clip(1e-300)
    for n in (0, 3):
        assert float(np.abs(got[:, :, :9, n].numpy()
                            - dipf[:, :, :9, n]).max()) < 1e-12


def test_argument_checks(sky):
    cent, dip = C.layouts()
    with pytest.raises(ValueError):
        beams.ArrayConfig(cent, C.LON, C.LAT, 0.0, S.DEC0, bf_type='tile')
    with pytest.raises(ValueError):
        beams.ArrayConfig(cent, C.LON, C.LAT, 0.0, S.DEC0, bf_type='hba',
                          tile_enu=dip)
    with pytest.raises(ValueError):          # 65 dipoles
        beams.ArrayConfig(cent, C.LON, C.LAT, 0.0, S.DEC0, bf_type='tile',
                          tile_enu=np.zeros((65, 3)))
    with pytest.raises(ValueError):          # per-station table, wrong N
        beams.ArrayConfig(cent, C.LON, C.LAT, 0.0, S.DEC0, bf_type='tile',
                          tile_enu=dip[:4])
    # D is not fixed at 16; a shared [D, 3] layout serves every station
    for nd in (1, 5, 64):
        c5, d5 = C.layouts(ndip=nd, shared=True)
        cfg = C.tile_cfg(c5, d5, 0.0, S.DEC0)
        geom = beams.beam_geometry(cfg, sky['ra'], sky['dec'], C.TMJD)
        got = beams.array_beam_gains(cfg, geom, S.FREQ0, 'cpu')
        ref = C.formula_gains(c5, d5, geom, [S.FREQ0])[0]
        assert float(np.abs(got.numpy() - ref).max()) < 1e-12
    # a geometry built for a single-stage config carries no du_tile
    cfg = C.tile_cfg(cent, dip, 0.0, S.DEC0)
    plain = beams.ArrayConfig(cent, C.LON, C.LAT, 0.0, S.DEC0)
    g1 = beams.beam_geometry(plain, sky['ra'], sky['dec'], C.TMJD)
    with pytest.raises(ValueError):
        beams.array_beam_gains(cfg, g1, S.FREQ0, 'cpu')


def test_tile_enu_alone_stays_single_stage(sky):
    """As tests/test_beams.py builds it: tile_enu set, type untouched."""
    cent, dip = C.layouts(tuple(C.TILES) + (5, 9, 33, 2))   # 10 stations
    plain = beams.ArrayConfig(cent, C.LON, C.LAT, 0.0, S.DEC0)
    cfg = beams.ArrayConfig(cent, C.LON, C.LAT, 0.0, S.DEC0, tile_enu=dip)
    assert cfg.bf_type == 'single'
    geom = beams.beam_geometry(cfg, sky['ra'], sky['dec'], C.TMJD)
    assert geom.du_tile is None
    g0 = beams.beam_geometry(plain, sky['ra'], sky['dec'], C.TMJD)
    assert torch.equal(beams.array_beam_gains(cfg, geom, S.FREQ0, 'cpu'),
                       beams.array_beam_gains(plain, g0, S.FREQ0, 'cpu'))
    args = (sky['pack'], *sky['uvw'], S.FREQ0, S.FREQ0, S.FDELTA, S.TDELTA,
            S.DEC0)
    tail = (C.TMJD, sky['bb'], sky['Nbase'], 3)
    assert torch.equal(beams.predict_coh_withbeam(*args, cfg, *tail, mode=1),
                       beams.predict_coh_withbeam(*args, plain, *tail,
                                                  mode=1))


TOL = 1e-10      # fp64 against fp64, max |err| / max |ref| per cluster


def _hand_built(sky, gains, ej=None):
    """sum_k g_p g_q E C_k E^H scattered to clusters, gains [T, K, N]."""
    pack, bb, Nbase = sky['pack'], sky['bb'], sky['Nbase']
    if ej is None:
        return S.beamed_reference(pack, range(pack.K), gains, bb, Nbase,
                                  *sky['uvw'], S.FREQ0)
    B = sky['uvw'][0].shape[0]
    t = torch.arange(B) // Nbase
    p, q = bb[:, 0].long(), bb[:, 1].long()
    co = pack.cluster_off.tolist()
    out = torch.zeros(pack.M, B, 2, 2, dtype=torch.complex128)
    for g in range(pack.K):
        ci = max(c for c in range(pack.M) if co[c] <= g)
        sub = beams._single_source_coh(pack, g, *sky['uvw'], S.FREQ0,
                                       S.FREQ0, S.FDELTA, S.TDELTA, S.DEC0)
        sub = ej[t, g] @ sub @ ej[t, g].conj().transpose(-1, -2)
        out[ci] += (gains[t, g, p] * gains[t, g, q])[:, None, None] * sub
    return out


@pytest.mark.parametrize('mode', [1, 2])
def test_predict_withbeam_two_stage(sky, mode):
    cent, dip = C.layouts(tuple(C.TILES) + (5, 9, 33, 2))   # 10 stations
    cfg = C.tile_cfg(cent, dip, 0.0, S.DEC0)
    plain = beams.ArrayConfig(cent, C.LON, C.LAT, 0.0, S.DEC0)
    geom = beams.beam_geometry(cfg, sky['ra'], sky['dec'], C.TMJD)
    gains = torch.from_numpy(C.formula_gains(cent, dip, geom, [S.FREQ0])[0])
    ej = None
    if mode == 2:
        coeffs = beams.make_synthetic_element_coeffs(freqs=(S.FREQ0,))
        ej = beams.element_jones(coeffs, geom, S.FREQ0)
    ref = _hand_built(sky, gains, ej)
    args = (sky['pack'], *sky['uvw'], S.FREQ0, S.FREQ0, S.FDELTA, S.TDELTA,
            S.DEC0)
    tail = (C.TMJD, sky['bb'], sky['Nbase'], 3)
    got = beams.predict_coh_withbeam(*args, cfg, *tail, mode=mode)
    err = S.cluster_err(got, ref)
    print(f'mode {mode} two-stage vs hand-built, per cluster:', err)
    assert max(err) < TOL, err
    # precomputed gains are used as given, with or without a tile config
    for c in (cfg, plain):
        again = beams.predict_coh_withbeam(*args, c, *tail, mode=mode,
                                           gains=gains)
        assert max(S.cluster_err(again, ref)) < TOL
    # a path that ignores the tiles must not pass
    single = beams.predict_coh_withbeam(*args, plain, *tail, mode=mode)
    gap = S.cluster_err(single, ref)
    print(f'mode {mode} single-stage vs two-stage, per cluster:', gap)
    assert min(gap) > 100 * TOL, gap


def test_mode3_ignores_the_beamformer_type(sky):
    cent, dip = C.layouts(tuple(C.TILES) + (5, 9, 33, 2))
    cfg = C.tile_cfg(cent, dip, 0.0, S.DEC0)
    plain = beams.ArrayConfig(cent, C.LON, C.LAT, 0.0, S.DEC0)
    args = (sky['pack'], *sky['uvw'], S.FREQ0, S.FREQ0, S.FDELTA, S.TDELTA,
            S.DEC0)
    tail = (C.TMJD, sky['bb'], sky['Nbase'], 3)
    assert torch.equal(beams.predict_coh_withbeam(*args, cfg, *tail, mode=3),
                       beams.predict_coh_withbeam(*args, plain, *tail,
                                                  mode=3))


# ---------------------------------------------------------------- CLI

WIDE_SKY = """\
A1 0 0 0 45 0 0 3.0 0 0 0 -0.7 0 0 0 0 150e6
A2 1 20 0 35 0 0 2.0 0 0 0 0.1 0 0 0 0 150e6
B1 23 0 0 52 0 0 2.5 0 0 0 -0.3 0 0 0 0 150e6
"""
WIDE_CLUSTER = "1 1 A1 A2\n2 1 B1\n"
NSTA = 8


def _beam_keys(seed=3):
    rng = np.random.default_rng(seed)
    grid = (np.arange(4) - 1.5) * 1.25
    gx, gy = np.meshgrid(grid, grid)
    dip = np.stack([np.column_stack([gx.ravel(), gy.ravel(), np.zeros(16)])
                    + rng.uniform(-0.05, 0.05, (16, 3))
                    for _ in range(NSTA)])
    return dict(element_enu=rng.uniform(-20, 20, (NSTA, 12, 3)),
                tile_enu=dip, tile_ra0=0.02, tile_dec0=np.pi / 4 - 0.014,
                lon=C.LON, lat=C.LAT, tmjd0=57000.0)


@pytest.fixture
def hba_obs(tmp_path):
    skyf, clf = tmp_path / 'sky.txt', tmp_path / 'cluster.txt'
    skyf.write_text(WIDE_SKY)
    clf.write_text(WIDE_CLUSTER)
    clusters = skymod.read_sky_cluster(str(skyf), str(clf), 0.0, np.pi / 4,
                                       150e6)
    pack = SourcePack(clusters)
    msf = str(tmp_path / 'hba.npz')
    msdata.make_synthetic_npz(msf, N=NSTA, tilesz=4, Ntime=4, Nchan=2,
                              pack=pack, bandwidth=50e3, noise_sigma=1e-3,
                              seed=5, ra0=0.0, dec0=np.pi / 4)
    z = dict(np.load(msf))
    z.update(_beam_keys())
    np.savez(msf, **z)
    return tmp_path, str(skyf), str(clf), msf, pack


@pytest.mark.parametrize('dobeam', [1, 5])
def test_cli_layer_matches_library(hba_obs, dobeam, monkeypatch):
    """_predict_with_beam on an npz with tile_enu is the library's
    two-stage predict; the gains of all channels come from ONE batched
    call per tile, shared by the solve predict and the residual path."""
    from sagecal_amd.apps import sagecal as app
    _, _, _, msf, pack = hba_obs
    calls = []
    real = beams.station_beam_gains

    def counted(cfg, geom, freqs, device='cpu'):
        calls.append(len(np.atleast_1d(freqs)))
        return real(cfg, geom, freqs, device)
    monkeypatch.setattr(beams, 'station_beam_gains', counted)
    args = types.SimpleNamespace(dobeam=dobeam, elem_type='auto')
    ms = msdata.NpzMS(msf, tilesz=4)
    tile = ms.load_tile(0)
    assert len(tile.freqs) == 2
    got = app._predict_with_beam(ms, pack, tile, 0, args)
    fd = tile.fdelta / 2
    chan = [app._predict_channel_with_beam(ms, pack, tile, 0, args,
                                           float(f), fd) for f in tile.freqs]
    # one batched call per tile serves both channels of every path; -B 1
    # evaluates the solve predict at the band centre first
    assert calls == ([2] if dobeam == 5 else [1, 2]), calls
    monkeypatch.setattr(beams, 'station_beam_gains', real)

    k = _beam_keys()
    cfg = beams.ArrayConfig(list(k['element_enu']), C.LON, C.LAT, 0.0,
                            np.pi / 4, tile_enu=k['tile_enu'],
                            bf_type='tile', tile_ra0=k['tile_ra0'],
                            tile_dec0=k['tile_dec0'])
    tmjd = 57000.0 + (np.arange(4) + 0.5) * ms.tdelta / 86400.0
    mode = dobeam if dobeam <= 3 else dobeam - 3

    def lib(c, f, fdelta):
        return beams.predict_coh_withbeam(
            pack, tile.u, tile.v, tile.w, f, tile.freq0, fdelta,
            tile.tdelta, tile.dec0, c, tmjd, ms.bb_tensor(), ms.Nbase, 4,
            mode=mode)
    per_chan = [lib(cfg, float(f), fd) for f in tile.freqs]
    ref = lib(cfg, tile.freq0, tile.fdelta) if dobeam <= 3 \
        else sum(per_chan) / 2
    assert max(S.cluster_err(got, ref)) < TOL
    for c, r in zip(chan, per_chan):
        assert max(S.cluster_err(c, r)) < TOL
    # and it is not the single-stage beam of the centroids
    plain = beams.ArrayConfig(list(k['element_enu']), C.LON, C.LAT, 0.0,
                              np.pi / 4)
    gap = S.cluster_err(lib(plain, float(tile.freqs[0]), fd), per_chan[0])
    assert min(gap) > 100 * TOL, gap


def test_cli_calibration_needs_the_tile_beam(hba_obs):
    """Simulate under the two-stage beam (-a 1 -B 1), then calibrate once
    with tile_enu in the MS and once with the key removed (every tile an
    isotropic element): the right model leaves the smaller residual."""
    from sagecal_amd.apps import sagecal as app
    tmp, skyf, clf, msf, _ = hba_obs
    rc = app.main(['-d', msf, '-s', skyf, '-c', clf, '-a', '1', '-t', '4',
                   '-B', '1', '-O', 'beamed'])
    assert rc == 0
    z = dict(np.load(msf))
    model = z.pop('beamed')
    assert np.abs(model).mean() > 1e-3
    rng = np.random.default_rng(2)
    z['data'] = (model + 1e-3 * (rng.standard_normal(model.shape)
                                 + 1j * rng.standard_normal(model.shape))
                 ).astype(model.dtype)
    res = {}
    for tag in ('tile', 'single'):
        f = str(tmp / f'{tag}.npz')
        zz = dict(z)
        if tag == 'single':
            for k in ('tile_enu', 'tile_ra0', 'tile_dec0'):
                del zz[k]
        np.savez(f, **zz)
        rc = app.main(['-d', f, '-s', skyf, '-c', clf, '-t', '4', '-e', '6',
                       '-g', '10', '-j', '3', '-l', '0', '-B', '1',
                       '-O', 'res'])
        assert rc == 0
        res[tag] = float(np.abs(np.load(f)['res']).mean())
    print('mean |residual|, right and wrong beam model:', res,
          'data:', float(np.abs(z['data']).mean()))
    assert res['tile'] < res['single'], res
