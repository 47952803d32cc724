"""k_element_beam, the device evaluation of the LOFAR dipole element
pattern at all channels in one launch, against the fp64 host
LofarElementCoeffs.eval, and the layers above it: hip_host.element_jones,
beams.element_jones_channels, predict_coh_withbeam modes 2/3 and the -B 5/6
command-line helpers.

Limits: max |err| <= 1e-5 * max |E_ref| per (table, frequency), the
project's kernel-versus-fp64 limit; 2e-4 per cluster GPU vs CPU
predict_coh_withbeam. A numpy float32 emulation of the kernel's arithmetic
gives 1.6e-7 to 3.4e-7 for the three tables and up to 4.7e-7 for M = 8.
Measured on an MI355X: 3.7e-7 at worst for the tables (see
test_kernel_matches_fp64_eval), 4.5e-7 for M = 8 with random
coefficients."""
import types

import numpy as np
import pytest
import torch

import shapelet_sky as S
from sagecal_amd import beams, msdata
from sagecal_amd.apps import sagecal as app
from sagecal_amd.ops import hip_host

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
N, T, K = 10, 3, 23
TMJD = np.array([57000.0, 57000.0001, 57000.0002])
LIMIT = 1e-5


def directions(t=T, k=K, seed=3):
    """az, el [t, k]: random above the horizon, then the special ones."""
    rng = np.random.default_rng(seed)
    az = rng.uniform(-np.pi, np.pi, (t, k))
    el = rng.uniform(0.0, np.pi / 2, (t, k))
    az[0, 0], el[0, 0] = 0.3, np.pi / 2        # zenith
    el[0, 1] = 0.0                             # on the horizon: above
    el[0, 2] = -1e-9                           # just below: exactly zero
    az[1, 0], az[1, 1] = np.pi, -np.pi
    el[2, 5] = -0.4
    return az, el


def fp64_eval(co, az, el, f):
    E = co.eval(np.pi / 2 - el.reshape(-1), az.reshape(-1), f)
    E[torch.from_numpy(el.reshape(-1) < 0)] = 0
    return E.reshape(*el.shape, 2, 2)


def table_freqs(co):
    """Below the table, on a node, between two nodes, above the table."""
    fr = co.freqs_ghz * 1e9
    return [0.5 * fr[0], fr[1], 0.3 * fr[1] + 0.7 * fr[2], 1.5 * fr[-1]]


def rel_err(got, ref):
    got = got.cpu().to(torch.complex128)
    return float((got - ref).abs().max() / ref.abs().max())


def random_coeffs(M, seed, beta=0.5):
    rng = np.random.default_rng(seed)
    nm = M * (M + 1) // 2
    c = rng.standard_normal((2, 2, nm)) + 1j * rng.standard_normal((2, 2, nm))
    return beams.LofarElementCoeffs(M, beta, [0.1, 0.2], c[0], c[1])


@pytest.mark.parametrize('kind', ['lba', 'hba', 'alo'])
def test_kernel_matches_fp64_eval(kind):
    """Measured on an MI355X, largest max |err| / max |E_ref| over the
    four frequencies at D = 69 and D = 270: lba 3.7e-7, hba 3.5e-7,
    alo 3.7e-7 (smallest 1.7e-7)."""
    co = beams.LofarElementCoeffs.load(kind)
    freqs = table_freqs(co)
    for shape in ((T, K), (3, 90)):            # D = 69; 270 = 5 blocks
        az, el = directions(*shape)
        got = hip_host.element_jones(co, az, el, freqs)
        assert got.is_cuda and got.dtype == torch.complex64
        assert got.shape == (4,) + shape + (2, 2)
        for i, f in enumerate(freqs):
            err = rel_err(got[i], fp64_eval(co, az, el, f))
            print(f'k_element_beam {kind} D={az.size} at {f:.6g} Hz: '
                  f'max err / max |E| = {err:.3g}')
            assert err <= LIMIT, (kind, f, err)
        g = got.cpu()
        assert not bool(g[:, 0, 2].any()) and not bool(g[:, 2, 5].any())
        assert bool((g[:, 0, 1].abs().amax(dim=(-1, -2)) > 0).all())


def test_batching_does_not_change_a_channel():
    co = beams.LofarElementCoeffs.load('hba')
    az, el = directions()
    fr = co.freqs_ghz * 1e9
    freqs = np.linspace(0.9 * fr[0], 1.1 * fr[-1], 70)   # > one LDS chunk
    big = hip_host.element_jones(co, az, el, freqs)
    assert big.shape == (70, T, K, 2, 2)
    assert torch.equal(big, hip_host.element_jones(co, az, el, freqs))
    three = hip_host.element_jones(co, az, el, freqs[[0, 16, 69]])
    for row, i in enumerate((0, 16, 69)):
        assert torch.equal(three[row], big[i])
    for i in (0, 15, 16, 17, 31, 32, 64, 69):
        one = hip_host.element_jones(co, az, el, [freqs[i]])
        assert one.shape == (1, T, K, 2, 2)
        assert torch.equal(one[0], big[i]), i


@pytest.mark.parametrize('M', [1, 2, 3, 8])
def test_general_mode_count(M):
    co = random_coeffs(M, seed=40 + M, beta=0.5 if M != 3 else 0.8)
    az, el = directions()
    freqs = [0.1e9, 0.16e9]
    got = hip_host.element_jones(co, az, el, freqs)
    for i, f in enumerate(freqs):
        err = rel_err(got[i], fp64_eval(co, az, el, f))
        print(f'k_element_beam M={M} at {f:.3g} Hz: {err:.3g}')
        assert err <= LIMIT, (M, f, err)


def test_mode_count_above_the_cap():
    az, el = directions()
    with pytest.raises(ValueError):
        hip_host.element_jones(random_coeffs(9, 1), az, el, [0.1e9])


def test_station_shaped_directions_feed_the_predict():
    """[T, K, N] directions give [F, T, K, N, 2, 2], the per-station
    `ejones` layout of hip_host.predict_coh (NE = N)."""
    pack, _ = S.make_pack()
    u, v, w, bb, Nbase = S.uvw_rows()
    co = beams.LofarElementCoeffs.load('lba')
    rng = np.random.default_rng(5)
    az = rng.uniform(-np.pi, np.pi, (T, pack.K, N))
    el = rng.uniform(-0.1, np.pi / 2, (T, pack.K, N))
    f = float(co.freqs_ghz[1] * 1e9)
    E = hip_host.element_jones(co, az, el, [f, 1.01 * f])
    assert E.shape == (2, T, pack.K, N, 2, 2)
    flat = hip_host.element_jones(co, az.reshape(-1), el.reshape(-1),
                                  [f, 1.01 * f])
    assert torch.equal(E.reshape(2, -1, 2, 2), flat)
    # a device tensor is taken as it is
    again = hip_host.element_jones(co, torch.as_tensor(az).to(DEV),
                                   torch.as_tensor(el).to(DEV), [f, 1.01 * f])
    assert torch.equal(again, E)
    pairs = bb[:Nbase].to(device=DEV, dtype=torch.int32)
    out = hip_host.predict_coh(pack, u.to(DEV), v.to(DEV), w.to(DEV),
                               S.FREQ0, S.FREQ0, S.FDELTA, S.TDELTA, S.DEC0,
                               pairs=pairs, Nbase=Nbase, ejones=E[0])
    assert out.shape == (pack.M, u.shape[0], 2, 2)
    assert bool(torch.isfinite(torch.view_as_real(out)).all())


@pytest.fixture(scope='module')
def sky():
    pack, _ = S.make_pack()
    u, v, w, bb, Nbase = S.uvw_rows()
    return dict(pack=pack, uvw=(u, v, w),
                uvw_d=tuple(x.to(DEV) for x in (u, v, w)), bb=bb,
                Nbase=Nbase)


def _cfg():
    rng = np.random.default_rng(7)
    elems = [rng.uniform(-30, 30, (16, 3)) for _ in range(N)]
    return beams.ArrayConfig(elems, 0.1, 0.92, 0.0, S.DEC0)


def _withbeam(sky, dev, mode, kind):
    uvw = sky['uvw'] if dev == 'cpu' else sky['uvw_d']
    return beams.predict_coh_withbeam(
        sky['pack'], *uvw, S.FREQ0, S.FREQ0, S.FDELTA, S.TDELTA, S.DEC0,
        _cfg(), TMJD, sky['bb'].to(dev), sky['Nbase'], T, mode=mode,
        coeffs=kind)


CASES = [(2, 'lba'), (3, 'lba'), (2, 'hba'), (3, 'hba')]


@pytest.fixture(scope='module')
def cpu_withbeam(sky):
    return {c: _withbeam(sky, 'cpu', *c) for c in CASES}


@pytest.mark.parametrize('case', CASES, ids=lambda c: f'mode{c[0]}-{c[1]}')
def test_withbeam_pattern_comes_from_the_device(sky, cpu_withbeam, case,
                                                monkeypatch):
    ref = cpu_withbeam[case]

    def boom(*a, **k):
        raise AssertionError('host element pattern evaluated on the GPU path')
    monkeypatch.setattr(beams.LofarElementCoeffs, 'basis', boom)
    got = _withbeam(sky, DEV, *case)
    assert got.is_cuda
    err = S.cluster_err(got, ref)
    print(f'withbeam mode {case[0]} {case[1]} gpu vs cpu, per cluster:', err)
    assert max(err) < 2e-4, err


@pytest.mark.parametrize('dobeam', [5, 6])
def test_wideband_cli_one_launch_per_tile(sky, monkeypatch, dobeam):
    calls = []
    real = hip_host.element_jones

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(hip_host, 'element_jones', counted)
    args = types.SimpleNamespace(dobeam=dobeam, elem_type='hba')
    enu = np.random.default_rng(7).uniform(-30, 30, (N, 16, 3))
    out, chan = {}, {}
    for dev in ('cpu', DEV):
        ms = msdata.SyntheticMS(N=N, tilesz=T, Ntime=T, Nchan=3, pack=None,
                                seed=13, device=dev)
        ms._z = {'element_enu': enu, 'lon': 0.1, 'lat': 0.92,
                 'tmjd0': 57000.0}
        tile = ms.load_tile(0)
        assert len(tile.freqs) == 3
        del calls[:]
        out[dev] = app._predict_with_beam(ms, sky['pack'], tile, 0, args)
        # the residual path of a tile channel reuses the tile's batch
        chan[dev] = app._predict_channel_with_beam(
            ms, sky['pack'], tile, 0, args, float(tile.freqs[2]),
            tile.fdelta / 3)
        assert len(calls) == (0 if dev == 'cpu' else 1), (dev, calls)
    assert out[DEV].is_cuda and chan[DEV].is_cuda
    for what, res in (('tile', out), ('one channel', chan)):
        err = S.cluster_err(res[DEV], res['cpu'])
        print(f'-B {dobeam} {what}, 3 channels, gpu vs cpu, per cluster:',
              err)
        assert max(err) < 2e-4, err


def test_argument_checks():
    co = beams.LofarElementCoeffs.load('hba')
    az, el = directions()
    f = float(co.freqs_ghz[0] * 1e9)
    with pytest.raises(ValueError):               # F = 0
        hip_host.element_jones(co, az, el, [])
    with pytest.raises(ValueError):               # az and el disagree
        hip_host.element_jones(co, az, el[:, :-1], [f])
    bad = beams.LofarElementCoeffs.load('hba')
    bad.theta = bad.theta[:, :-1]
    bad.phi = bad.phi[:, :-1]
    with pytest.raises(ValueError):               # width is not M(M+1)/2
        hip_host.element_jones(bad, az, el, [f])

    ext = hip_host._ext()
    dev = torch.device(DEV)
    nm = co.Nmodes
    a = torch.zeros(5, dtype=torch.float64, device=dev)
    coef = torch.zeros(2, 2, nm, dtype=torch.complex64, device=dev)
    pre = torch.ones(nm, dtype=torch.float32, device=dev)
    ok = ext.element_jones(a, a, coef, pre, co.M, co.beta)
    assert ok.shape == (2, 5, 2, 2)               # the inputs are sound
    refused = {
        'CPU az': (a.cpu(), a, coef, pre, co.M, co.beta),
        'CPU coef': (a, a, coef.cpu(), pre, co.M, co.beta),
        'float32 az': (a.float(), a, coef, pre, co.M, co.beta),
        'complex128 coef': (a, a, coef.to(torch.complex128), pre, co.M,
                            co.beta),
        'float64 preamble': (a, a, coef, pre.double(), co.M, co.beta),
        'el shorter than az': (a, a[:4], coef, pre, co.M, co.beta),
        'coef for another M': (a, a, coef, pre, co.M - 1, co.beta),
        'no frequency': (a, a, coef[:0], pre, co.M, co.beta),
        'M above the cap': (a, a, torch.zeros(1, 2, 45, dtype=torch.complex64,
                                              device=dev),
                            torch.ones(45, dtype=torch.float32, device=dev),
                            9, co.beta),
        'beta = 0': (a, a, coef, pre, co.M, 0.0),
    }
    for what, call in refused.items():
        with pytest.raises(RuntimeError):
            ext.element_jones(*call)
            pytest.fail(f'the extension accepted: {what}')
