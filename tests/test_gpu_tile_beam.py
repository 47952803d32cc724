"""k_station_beam, the frequency-batched single- and two-stage station beam
kernel, against the fp64 CPU gains, and beams.predict_coh_withbeam modes 1
and 2 of a two-stage config on the GPU against the CPU per-source loop.

Limits: 2e-5 absolute for two-stage gains (each factor is a gain <= 1 that
test_array_beam_kernel holds to 1e-5 at these element counts, and
|d(ab)| <= |da| + |db|), 1e-5 for single-stage gains, 2e-4 max |err| /
max |ref| per cluster for the predict, as the single-stage tests use."""
import numpy as np
import pytest
import torch

import shapelet_sky as S
import tile_beam_cases as C
from sagecal_amd import beams
from sagecal_amd.ops import hip_host

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
T = 3
FREQS = [120e6, 150e6, 180e6]


def _directions(K, b_ra0=0.0, b_dec0=S.DEC0, seed=5):
    """K - 1 sources around the pointing, the last one under the horizon."""
    rng = np.random.default_rng(seed)
    ra = np.concatenate([b_ra0 + rng.uniform(-0.3, 0.3, K - 1),
                         [b_ra0 + np.pi]])
    dec = np.concatenate([b_dec0 + rng.uniform(-0.25, 0.25, K - 1),
                          [-b_dec0]])
    return ra, dec


@pytest.fixture(scope='module', params=[10, 90], ids=['K10', 'K90'])
def case(request):
    """T*K = 30 is under one block of 256 (t,k); 270 spans two. The fp64
    CPU gains are computed once per K."""
    K = request.param
    cent, dip = C.layouts()
    cfg = C.tile_cfg(cent, dip, 0.0, S.DEC0)
    plain = beams.ArrayConfig(cent, C.LON, C.LAT, 0.0, S.DEC0)
    ra, dec = _directions(K)
    geom = beams.beam_geometry(cfg, ra, dec, C.TMJD)
    assert not geom.below[:, :K - 1].any() and geom.below[:, K - 1].all()
    return dict(K=K, cent=cent, dip=dip, cfg=cfg, plain=plain, geom=geom,
                ref=beams.station_beam_gains(cfg, geom, FREQS, 'cpu'),
                ref1=beams.station_beam_gains(plain, geom, FREQS, 'cpu'))


def test_kernel_matches_fp64_gains(case):
    K, N = case['K'], len(C.TILES)
    got = beams.station_beam_gains(case['cfg'], case['geom'], FREQS, DEV)
    assert got.is_cuda and got.dtype == torch.float32
    assert got.shape == (3, T, K, N)
    diff = float((got.cpu().double() - case['ref']).abs().max())
    print(f'k_station_beam two-stage vs fp64, K={K}, max abs diff:', diff)
    assert diff < 2e-5, diff
    gap = float((case['ref'] - case['ref1']).abs().max())
    assert gap > 0.1, gap          # the tile factor is not a no-op here
    one = beams.station_beam_gains(case['plain'], case['geom'], FREQS, DEV)
    diff = float((one.cpu().double() - case['ref1']).abs().max())
    print(f'k_station_beam single-stage vs fp64, K={K}, max abs diff:', diff)
    assert diff < 1e-5, diff
    # below the horizon: exactly 0; one-tile station, single stage: exactly 1
    assert bool((got[:, :, K - 1, :] == 0).all())
    assert bool((one[:, :, K - 1, :] == 0).all())
    assert bool((one[:, :, :K - 1, 0] == 1).all())
    # array_beam_gains of a tile config is the one-frequency launch
    g1 = beams.array_beam_gains(case['cfg'], case['geom'], FREQS[1], DEV)
    assert g1.shape == (T, K, N)
    assert float((g1.cpu().double() - case['ref'][1]).abs().max()) < 2e-5


def test_frequency_rows_are_independent(case):
    cfg, geom = case['cfg'], case['geom']
    got = beams.station_beam_gains(cfg, geom, FREQS, DEV)
    assert torch.equal(got, beams.station_beam_gains(cfg, geom, FREQS, DEV))
    for fi, f in enumerate(FREQS):
        alone = beams.station_beam_gains(cfg, geom, [f], DEV)
        assert alone.shape[0] == 1
        assert torch.equal(alone[0], got[fi]), f
    # more rows than one thread carries per pass, in another order
    many = FREQS[::-1] + [135e6, 165e6, 150e6]
    rows = beams.station_beam_gains(cfg, geom, many, DEV)
    for fi, f in enumerate(many):
        if f in FREQS:
            assert torch.equal(rows[fi], got[FREQS.index(f)]), (fi, f)
    assert torch.equal(rows[5], rows[1])


def test_zero_dipole_offsets_give_the_centroid_beam(case):
    """Every dipole at the tile centre: the tile factor is 1 and the gains
    are those of k_array_beam on the centroids, within 1e-5."""
    cfg0 = C.tile_cfg(case['cent'], np.zeros((len(C.TILES), C.D, 3)), 0.0,
                      S.DEC0)
    got = beams.station_beam_gains(cfg0, case['geom'], FREQS, DEV)
    for fi, f in enumerate(FREQS):
        ref = beams.array_beam_gains(case['plain'], case['geom'], f, DEV)
        diff = float((got[fi] - ref).abs().max())
        print(f'zero dipoles vs k_array_beam at {f:.4g} Hz:', diff)
        assert diff < 1e-5, diff
    one_tile = got[:, :, :case['K'] - 1, 0]
    assert float((one_tile - 1).abs().max()) < 1e-6


# ------------------------------------------------------------ predict

N10 = tuple(C.TILES) + (5, 9, 33, 2)        # the 10 stations of the rows


@pytest.fixture(scope='module')
def sky():
    pack, _ = S.make_pack()
    u, v, w, bb, Nbase = S.uvw_rows()
    cent, dip = C.layouts(N10)
    return dict(pack=pack, uvw=(u, v, w), bb=bb, Nbase=Nbase,
                uvw_d=tuple(x.to(DEV) for x in (u, v, w)),
                cfg=C.tile_cfg(cent, dip, 0.0, S.DEC0),
                plain=beams.ArrayConfig(cent, C.LON, C.LAT, 0.0, S.DEC0))


def _withbeam(sky, dev, mode, cfg, **kw):
    uvw = sky['uvw'] if dev == 'cpu' else sky['uvw_d']
    return beams.predict_coh_withbeam(
        sky['pack'], *uvw, S.FREQ0, S.FREQ0, S.FDELTA, S.TDELTA, S.DEC0,
        cfg, C.TMJD, sky['bb'].to(dev), sky['Nbase'], T, mode=mode, **kw)


@pytest.fixture(scope='module')
def cpu_withbeam(sky):
    return {m: _withbeam(sky, 'cpu', m, sky['cfg']) for m in (1, 2)}


@pytest.mark.parametrize('mode', [1, 2])
def test_withbeam_two_stage_gpu_matches_cpu(sky, cpu_withbeam, mode,
                                            monkeypatch):
    """GPU vs the CPU loop; the device path runs neither the per-source
    loop nor the torch array factor."""
    def boom(*a, **k):
        raise AssertionError('host beam code called on the GPU path')
    monkeypatch.setattr(beams, '_single_source_coh', boom)
    monkeypatch.setattr(beams, 'array_beam', boom)
    monkeypatch.setattr(beams, '_array_factor', boom)
    got = _withbeam(sky, DEV, mode, sky['cfg'])
    assert got.is_cuda
    err = S.cluster_err(got, cpu_withbeam[mode])
    print(f'two-stage withbeam mode {mode} gpu vs cpu, per cluster:', err)
    assert max(err) < 2e-4, err
    # gains handed in (one row of a batch) give the same call
    geom = beams.beam_geometry(sky['cfg'],
                               *beams._pack_radec(sky['pack'], S.DEC0),
                               C.TMJD)
    rows = beams.station_beam_gains(sky['cfg'], geom,
                                    [0.98 * S.FREQ0, S.FREQ0], DEV)
    again = _withbeam(sky, DEV, mode, sky['cfg'], geom=geom, gains=rows[1])
    assert torch.equal(again, got)
    # the single-stage beam of the centroids is well outside the limit
    single = _withbeam(sky, DEV, mode, sky['plain'])
    gap = S.cluster_err(single, cpu_withbeam[mode])
    assert min(gap) > 10 * 2e-4, gap


def test_host_argument_checks(monkeypatch):
    """Every one raises on the host before the extension is reached, so
    before any launch."""
    K = 4
    elem = torch.zeros(2, 4, 3, dtype=torch.float64, device=DEV)
    tile = torch.zeros(2, 16, 3, dtype=torch.float64, device=DEV)
    du = torch.zeros(T, K, 3, dtype=torch.float64)
    below = torch.zeros(T, K, dtype=torch.uint8)
    ne = np.array([4, 2])
    ok = hip_host.station_beam_gains(elem, ne, du, below, FREQS, tile=tile,
                                     du_tile=du)
    assert ok.shape == (3, T, K, 2)
    assert float((ok - 1).abs().max()) < 1e-6      # every phasor is 1
    bad = [
        dict(nelem=np.array([4, 0])),                    # empty station
        dict(nelem=np.array([4, 5])),                    # nelem > Emax
        dict(nelem=np.array([4])),                       # wrong length
        dict(elem=elem.cpu()),                           # host tensor
        dict(elem=elem[:, :, :2]),                       # not [., ., 3]
        dict(below=below[:, :3]),                        # below vs du
        dict(du_tile=None),                              # tile alone
        dict(tile=None),                                 # du_tile alone
        dict(tile=tile.cpu()),                           # tile on the host
        dict(tile=tile[:1]),                             # wrong N
        dict(tile=torch.zeros(2, 65, 3, dtype=torch.float64, device=DEV)),
        dict(du_tile=du[:, :3]),                         # shape vs du
        dict(freqs=[]),                                  # no frequency
    ]
    def boom():
        raise AssertionError('extension reached with bad arguments')
    monkeypatch.setattr(hip_host, '_ext', boom)
    for kw in bad:
        a = dict(elem=elem, nelem=ne, du=du, below=below, freqs=FREQS,
                 tile=tile, du_tile=du)
        a.update(kw)
        with pytest.raises(ValueError):
            hip_host.station_beam_gains(**a)
