"""Element and array station beams inside the HIP predict kernels: the
E-Jones sandwich of k_predict_coh_ej / k_shapelet_coh_ej, the device array
factor k_array_beam, and beams.predict_coh_withbeam modes 1-3 on the GPU
against the CPU per-source loop. Limits are max |err| / max |ref| per
cluster: 1e-5 kernel vs fp64, 2e-4 GPU vs CPU predict_coh_withbeam."""
import types

import numpy as np
import pytest
import torch

import shapelet_sky as S
from sagecal_amd import beams
from sagecal_amd.ops import hip_host

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
N, T = 10, 3
TMJD = np.array([57000.0, 57000.0001, 57000.0002])


def _cfg(lat=0.92):
    rng = np.random.default_rng(7)
    elems = [rng.uniform(-30, 30, (16, 3)) for _ in range(N)]
    return beams.ArrayConfig(elems, 0.1, lat, 0.0, S.DEC0)


def _random_e(K, seed):
    """[T, K, N, 2, 2] complex64, re/im uniform in +-1, all different."""
    rng = np.random.default_rng(seed)
    e = rng.uniform(-1, 1, (T, K, N, 2, 2)) \
        + 1j * rng.uniform(-1, 1, (T, K, N, 2, 2))
    return torch.tensor(e, dtype=torch.complex64)


def _random_beam(K, seed):
    rng = np.random.default_rng(seed)
    return torch.tensor(rng.uniform(0.2, 1.0, (T, K, N)),
                        dtype=torch.float32)


def _sandwich_reference(pack, ejones, beam, bb, Nbase, u, v, w, freq):
    """fp64 sum over sources of g_p g_q E_p C_k E_q^H scattered to the
    clusters: [M, B, 2, 2] complex128. ejones [T, K, NE, 2, 2]."""
    B = u.shape[0]
    t = torch.arange(B) // Nbase
    p, q = bb[:, 0].long(), bb[:, 1].long()
    co = pack.cluster_off.tolist()
    E = ejones.to(torch.complex128)
    if E.shape[2] == 1:
        E = E.expand(-1, -1, N, -1, -1)
    out = torch.zeros(pack.M, B, 2, 2, dtype=torch.complex128)
    for g in range(pack.K):
        ci = max(c for c in range(pack.M) if co[c] <= g)
        sub = beams._single_source_coh(pack, g, u, v, w, freq, S.FREQ0,
                                       S.FDELTA, S.TDELTA, S.DEC0)
        sub = E[t, g, p] @ sub.to(torch.complex128) \
            @ E[t, g, q].conj().transpose(-1, -2)
        if beam is not None:
            bd = beam.to(torch.float64)
            sub = (bd[t, g, p] * bd[t, g, q])[:, None, None] * sub
        out[ci] += sub
    return out


@pytest.fixture(scope='module')
def sky():
    pack, gis = S.make_pack()
    u, v, w, bb, Nbase = S.uvw_rows()
    uvw_d = tuple(x.to(DEV) for x in (u, v, w))
    pairs = bb[:Nbase].to(device=DEV, dtype=torch.int32)
    return dict(pack=pack, gis=gis, uvw=(u, v, w), uvw_d=uvw_d, bb=bb,
                Nbase=Nbase, pairs=pairs, ej=_random_e(pack.K, 21),
                beam=_random_beam(pack.K, 22))


def _gpu_predict(sky, pack=None, **kw):
    for k in ('beam', 'ejones'):
        if kw.get(k) is not None:
            kw[k] = kw[k].to(DEV)
    return hip_host.predict_coh(pack or sky['pack'], *sky['uvw_d'], S.FREQ0,
                                S.FREQ0, S.FDELTA, S.TDELTA, S.DEC0, **kw)


@pytest.mark.parametrize('with_beam', [False, True], ids=['mode3', 'mode2'])
def test_kernel_with_given_ejones(sky, with_beam):
    """Distinct complex E per (t, k, station): a p/q swap, a transpose for
    the conjugate transpose, a wrong timeslot or source index all show."""
    beam = sky['beam'] if with_beam else None
    ref = _sandwich_reference(sky['pack'], sky['ej'], beam, sky['bb'],
                              sky['Nbase'], *sky['uvw'], S.FREQ0)
    got = _gpu_predict(sky, ejones=sky['ej'], beam=beam, pairs=sky['pairs'],
                       Nbase=sky['Nbase'])
    err = S.cluster_err(got, ref)
    print('E-Jones kernel vs fp64 per-source sum, per cluster:', err)
    assert max(err) < 1e-5, err
    again = _gpu_predict(sky, ejones=sky['ej'], beam=beam,
                         pairs=sky['pairs'], Nbase=sky['Nbase'])
    assert torch.equal(got, again)


def test_single_pattern_broadcasts(sky):
    one = sky['ej'][:, :, :1].contiguous()
    full = one.expand(-1, -1, N, -1, -1).contiguous()
    kw = dict(beam=sky['beam'], pairs=sky['pairs'], Nbase=sky['Nbase'])
    got = _gpu_predict(sky, ejones=one, **kw)
    ref = _gpu_predict(sky, ejones=full, **kw)
    err = S.cluster_err(got, ref)
    print('NE=1 vs NE=N, per cluster:', err)
    assert max(err) < 1e-5, err
    fp64 = _sandwich_reference(sky['pack'], one, sky['beam'], sky['bb'],
                               sky['Nbase'], *sky['uvw'], S.FREQ0)
    err = S.cluster_err(got, fp64)
    print('NE=1 vs fp64, per cluster:', err)
    assert max(err) < 1e-5, err


def test_identity_ejones_is_the_plain_predict(sky):
    eye = torch.eye(2, dtype=torch.complex64).expand(T, sky['pack'].K, 1,
                                                     2, 2).contiguous()
    got = _gpu_predict(sky, ejones=eye, pairs=sky['pairs'],
                       Nbase=sky['Nbase'])
    ref = _gpu_predict(sky)
    err = S.cluster_err(got, ref)
    print('identity E vs plain predict, per cluster:', err)
    assert max(err) < 1e-5, err


def test_source_tile_boundary(sky):
    """70 sources per cluster: cluster 0 crosses the 64-source LDS tile,
    cluster 1 starts at offset 70."""
    pack, _ = S.make_pack(spec=(), M=2, nsrc=70)
    ej, beam = _random_e(pack.K, 23), _random_beam(pack.K, 24)
    ref = _sandwich_reference(pack, ej, beam, sky['bb'], sky['Nbase'],
                              *sky['uvw'], S.FREQ0)
    got = _gpu_predict(sky, pack=pack, ejones=ej, beam=beam,
                       pairs=sky['pairs'], Nbase=sky['Nbase'])
    err = S.cluster_err(got, ref)
    print('140 sources, E-Jones kernel vs fp64, per cluster:', err)
    assert max(err) < 1e-5, err


def test_array_beam_kernel(sky):
    counts = [1, 5, 16, 64, 65, 96, 16, 16, 16, 16]
    rng = np.random.default_rng(31)
    elems = [rng.uniform(-30, 30, (c, 3)) for c in counts]
    cfg = beams.ArrayConfig(elems, 0.1, 0.92, 0.0, S.DEC0)
    ra, dec = beams._pack_radec(sky['pack'], S.DEC0)
    ra = np.concatenate([ra, [cfg.b_ra0 + np.pi]])
    dec = np.concatenate([dec, [-cfg.b_dec0]])
    geom = beams.beam_geometry(cfg, ra, dec, TMJD)
    assert not geom.below[:, :9].any() and geom.below[:, 9].all()
    for freq in (S.FREQ0, 1.02 * S.FREQ0):
        ref = beams.array_beam_gains(cfg, geom, freq, 'cpu')
        got = beams.array_beam_gains(cfg, geom, freq, DEV)
        assert got.is_cuda and got.dtype == torch.float32
        assert got.shape == (T, 10, N)
        diff = float((got.cpu().double() - ref).abs().max())
        print(f'k_array_beam vs fp64 at {freq:.4g} Hz, max abs diff:', diff)
        assert diff < 1e-5, diff
        assert bool((got[:, 9, :] == 0).all())          # below the horizon
        assert bool((got[:, :9, 0] == 1).all())         # one element
        again = beams.array_beam_gains(cfg, geom, freq, DEV)
        assert torch.equal(got, again)


def _withbeam(sky, dev, mode, cfg, coeffs=None):
    uvw = sky['uvw'] if dev == 'cpu' else sky['uvw_d']
    return beams.predict_coh_withbeam(
        sky['pack'], *uvw, S.FREQ0, S.FREQ0, S.FDELTA, S.TDELTA, S.DEC0,
        cfg, TMJD, sky['bb'].to(dev), sky['Nbase'], T, mode=mode,
        coeffs=coeffs)


CASES = [(1, None), (2, None), (3, None), (2, 'lba')]


@pytest.fixture(scope='module')
def cpu_withbeam(sky):
    """CPU per-source loop results, computed once per (mode, coeffs)."""
    cfg = _cfg()
    return {c: _withbeam(sky, 'cpu', c[0], cfg, c[1]) for c in CASES}


@pytest.mark.parametrize('case', CASES,
                         ids=['mode1', 'mode2', 'mode3', 'mode2-lba'])
def test_withbeam_gpu_matches_cpu(sky, cpu_withbeam, case):
    got = _withbeam(sky, DEV, case[0], _cfg(), case[1])
    assert got.is_cuda
    err = S.cluster_err(got, cpu_withbeam[case])
    print(f'withbeam mode {case[0]} {case[1] or "synthetic"} gpu vs cpu, '
          'per cluster:', err)
    assert max(err) < 2e-4, err


@pytest.mark.parametrize('mode', [1, 2, 3])
def test_withbeam_all_below_horizon_is_zero(sky, mode):
    cfg = _cfg(lat=-0.92)
    cpu = _withbeam(sky, 'cpu', mode, cfg)
    gpu = _withbeam(sky, DEV, mode, cfg)
    assert not cpu.any() and not gpu.any()


def test_withbeam_no_host_loop(sky, cpu_withbeam, monkeypatch):
    """The GPU path never runs the per-source loop or the torch array
    factor."""
    def boom(*a, **k):
        raise AssertionError('host beam code called on the GPU path')
    monkeypatch.setattr(beams, '_single_source_coh', boom)
    monkeypatch.setattr(beams, 'array_beam', boom)
    for mode in (1, 2, 3):
        got = _withbeam(sky, DEV, mode, _cfg())
        err = S.cluster_err(got, cpu_withbeam[(mode, None)])
        assert max(err) < 2e-4, (mode, err)


def test_wideband_cli_layer_builds_geometry_once(sky, monkeypatch):
    """-B 5 (per-channel array+element beam) through the CLI helper: the
    geometry is built once per tile, not once per channel."""
    from sagecal_amd import msdata
    from sagecal_amd.apps import sagecal as app
    calls = []
    real = beams.beam_geometry

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(beams, 'beam_geometry', counted)
    args = types.SimpleNamespace(dobeam=5, elem_type='auto')
    enu = np.random.default_rng(7).uniform(-30, 30, (N, 16, 3))
    out = {}
    for dev in ('cpu', DEV):
        ms = msdata.SyntheticMS(N=N, tilesz=T, Ntime=T, Nchan=2, pack=None,
                                seed=13, device=dev)
        ms._z = {'element_enu': enu, 'lon': 0.1, 'lat': 0.92,
                 'tmjd0': 57000.0}
        tile = ms.load_tile(0)
        assert len(tile.freqs) == 2
        del calls[:]
        out[dev] = app._predict_with_beam(ms, sky['pack'], tile, 0, args)
        assert len(calls) == 1, calls
    assert out[DEV].is_cuda
    err = S.cluster_err(out[DEV], out['cpu'])
    print('-B 5 two channels gpu vs cpu, per cluster:', err)
    assert max(err) < 2e-4, err


def test_argument_checks(sky):
    K = sky['pack'].K
    kw = dict(pairs=sky['pairs'], Nbase=sky['Nbase'])
    with pytest.raises(ValueError):           # NE not in {1, N}
        _gpu_predict(sky, ejones=sky['ej'][:, :, :3].contiguous(), **kw)
    with pytest.raises(ValueError):           # T * Nbase != R
        _gpu_predict(sky, ejones=sky['ej'][:2].contiguous(), **kw)
    with pytest.raises(ValueError):           # no pairs
        _gpu_predict(sky, ejones=sky['ej'], Nbase=sky['Nbase'])
    with pytest.raises(ValueError):           # fewer sources than the pack
        _gpu_predict(sky, ejones=sky['ej'][:, :K - 1].contiguous(), **kw)
    elem = torch.zeros(2, 4, 3, dtype=torch.float64, device=DEV)
    du = torch.zeros(T, K, 3, dtype=torch.float64)
    below = torch.zeros(T, K, dtype=torch.uint8)
    with pytest.raises(ValueError):           # a station with no elements
        hip_host.array_beam_gains(elem, np.array([4, 0]), du, below, S.FREQ0)


def test_extension_rejects_malformed_beam(sky):
    """The extension's predict_coh and shapelet_coh_add, called directly
    (hip_host casts and slices before it calls them), refuse a beam or a
    pair table the kernels would index out of bounds: 3 stations, 1
    timeslot, 2 point sources, R = 3 rows. Each call returns before any
    launch. shapelet_coh_add gets the mode table of the module's sky; its
    checks never get as far as relating the table to the beam."""
    ext = hip_host._ext()
    dev = torch.device(DEV)
    pack, _ = S.make_pack(spec=(), M=2, nsrc=1)
    gp = hip_host.gpu_pack(pack, dev)
    assert gp.K == 2 and gp.sh is None and not bool(gp.stype.any())
    u, v, w = (x[:3].contiguous() for x in sky['uvw_d'])
    Nbase = 3
    pairs = torch.tensor([[0, 1], [0, 2], [1, 2]], dtype=torch.int32,
                         device=dev)
    beam = torch.full((1, 2, 3), 0.5, dtype=torch.float32, device=dev)
    sI, sQ, sU, sV = gp.fluxes_at(S.FREQ0, S.FREQ0)
    r1 = gp.r1_for(S.DEC0)
    chan = (S.FREQ0, S.FDELTA * 0.5, S.TDELTA)

    def predict(beam, pairs):
        return ext.predict_coh(
            u, v, w, gp.ll, gp.mm, gp.nn1, sI, sQ, sU, sV, gp.eX, gp.eY,
            gp.eP, gp.cxi, gp.sxi, gp.cphi, gp.sphi, r1, gp.stype,
            gp.cluster_off, *chan, beam=beam, pairs=pairs, Nbase=Nbase)

    sgp = hip_host.gpu_pack(sky['pack'], dev)
    tab = sgp.sh
    flux = sgp.shapelet_fluxes_at(S.FREQ0, S.FREQ0)
    r1s = sgp.r1_for(S.DEC0).index_select(0, tab.src)
    out = torch.zeros(sgp.M, 3, 4, dtype=torch.complex64, device=dev)

    def shapelet_add(beam, pairs):
        ext.shapelet_coh_add(
            out, u, v, w, *(getattr(tab, k) for k in tab.FIELDS), flux, r1s,
            *chan, beam=beam, pairs=pairs, Nbase=Nbase)

    assert predict(beam, pairs).shape == (2, 3, 4)    # the inputs are sound
    bad = {'float64 beam': (beam.double(), pairs),
           'CPU beam': (beam.cpu(), pairs),
           'T*Nbase < R': (beam[:0].contiguous(), pairs),
           '2*Nbase - 1 pair entries': (beam, pairs.reshape(-1)[:5]
                                        .contiguous())}
    for call in (predict, shapelet_add):
        for what, (b, p) in bad.items():
            with pytest.raises(RuntimeError):
                call(b, p)
                pytest.fail(f'{call.__name__} accepted a {what}')
    assert not bool(out.any())                        # nothing was added
