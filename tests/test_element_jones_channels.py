"""beams.element_jones_channels on the CPU, the `ejones=` keyword of
predict_coh_withbeam, and the per-tile batching of the element pattern in
the -B 5/6 command-line helpers. No GPU needed."""
import types

import numpy as np
import pytest
import torch

import shapelet_sky as S
from sagecal_amd import beams, msdata
from sagecal_amd.apps import sagecal as app

N, T = 10, 3
TMJD = np.array([57000.0, 57000.0001, 57000.0002])


def _cfg():
    rng = np.random.default_rng(7)
    elems = [rng.uniform(-30, 30, (16, 3)) for _ in range(N)]
    return beams.ArrayConfig(elems, 0.1, 0.92, 0.0, S.DEC0)


def table_freqs(co):
    """Below the table, on a node, between two nodes, above the table."""
    fr = co.freqs_ghz * 1e9
    return [0.5 * fr[0], fr[1], 0.3 * fr[1] + 0.7 * fr[2], 1.5 * fr[-1]]


@pytest.fixture(scope='module')
def sky():
    pack, _ = S.make_pack()
    u, v, w, bb, Nbase = S.uvw_rows()
    return dict(pack=pack, uvw=(u, v, w), bb=bb, Nbase=Nbase)


@pytest.fixture(scope='module')
def geom(sky):
    """The pack's sources plus one below the horizon."""
    cfg = _cfg()
    ra, dec = beams._pack_radec(sky['pack'], S.DEC0)
    ra = np.concatenate([ra, [cfg.b_ra0 + np.pi]])
    dec = np.concatenate([dec, [-cfg.b_dec0]])
    g = beams.beam_geometry(cfg, ra, dec, TMJD)
    assert not g.below[:, :-1].any() and g.below[:, -1].all()
    return g


@pytest.mark.parametrize('kind', ['lba', 'hba', 'alo', 'synthetic'])
def test_channels_are_the_per_frequency_stack(geom, kind):
    if kind == 'synthetic':
        co = beams.make_synthetic_element_coeffs(freqs=(120e6, 150e6, 180e6))
        freqs = [100e6, 150e6, 166e6, 200e6]
    else:
        co = beams.LofarElementCoeffs.load(kind)
        freqs = table_freqs(co)
    got = beams.element_jones_channels(co, geom, freqs, 'cpu')
    assert got.shape == (4, geom.T, geom.K, 2, 2)
    assert got.dtype == torch.complex128
    for i, f in enumerate(freqs):
        assert torch.equal(got[i], beams.element_jones(co, geom, f)), (kind, f)
    assert not bool(got[:, :, -1].any())          # below the horizon
    assert bool(got[:, :, :-1].abs().amax(dim=(-1, -2)).min() > 0)
    one = beams.element_jones_channels(co, geom, freqs[2])
    assert torch.equal(one, got[2:3])


def test_channels_reject_empty_freqs(geom):
    with pytest.raises(ValueError):
        beams.element_jones_channels('hba', geom, [])


def _withbeam(sky, mode, coeffs, **kw):
    return beams.predict_coh_withbeam(
        sky['pack'], *sky['uvw'], S.FREQ0, S.FREQ0, S.FDELTA, S.TDELTA,
        S.DEC0, _cfg(), TMJD, sky['bb'], sky['Nbase'], T, mode=mode,
        coeffs=coeffs, **kw)


@pytest.mark.parametrize('mode', [2, 3])
@pytest.mark.parametrize('coeffs', ['hba', None], ids=['hba', 'synthetic'])
def test_given_ejones_equals_computed(sky, mode, coeffs):
    """Handed the E-Jones that the call evaluates itself, timeslot by
    timeslot, the result is the same to the bit. Handed the one evaluation
    over all T*K directions (what element_jones_channels gives), it agrees
    to 1e-14: the matrix-vector products run over another number of rows,
    which a BLAS may sum in another order."""
    cfg = _cfg()
    g = beams.beam_geometry(cfg, *beams._pack_radec(sky['pack'], S.DEC0),
                            TMJD)
    ref = _withbeam(sky, mode, coeffs)
    assert bool(ref.any())
    co = beams._resolve_coeffs(coeffs, S.FREQ0)
    per_slot = torch.stack([
        beams.element_beam(co, g.az[t], np.maximum(g.el[t], 0.0), S.FREQ0)
        for t in range(g.T)])
    assert not g.below.any()
    assert torch.equal(_withbeam(sky, mode, coeffs, ejones=per_slot), ref)
    E = beams.element_jones_channels(coeffs, g, [S.FREQ0])[0]
    got = _withbeam(sky, mode, coeffs, ejones=E)
    err = S.cluster_err(got, ref)
    print(f'mode {mode} ejones= given vs computed, per cluster:', err)
    assert max(err) <= 1e-14, err
    # not read when the E-Jones is given
    again = _withbeam(sky, mode, 'no-such-table', ejones=E)
    assert torch.equal(again, got)


@pytest.mark.parametrize('dobeam', [5, 6])
def test_wideband_cli_evaluates_pattern_once_per_tile(sky, monkeypatch,
                                                      dobeam):
    """-B 5/6 with the HBA table on a 3-channel tile: one batched pattern
    evaluation per tile, the result of the channel-by-channel path."""
    calls = []
    real = beams.element_jones_channels

    def counted(coeffs, geom, freqs, device='cpu'):
        calls.append(len(np.atleast_1d(freqs)))
        return real(coeffs, geom, freqs, device)
    monkeypatch.setattr(beams, 'element_jones_channels', counted)
    args = types.SimpleNamespace(dobeam=dobeam, elem_type='hba')
    enu = np.random.default_rng(7).uniform(-30, 30, (N, 16, 3))
    ms = msdata.SyntheticMS(N=N, tilesz=T, Ntime=T, Nchan=3, pack=None,
                            seed=13)
    ms._z = {'element_enu': enu, 'lon': 0.1, 'lat': 0.92, 'tmjd0': 57000.0}
    tile = ms.load_tile(0)
    assert len(tile.freqs) == 3
    got = app._predict_with_beam(ms, sky['pack'], tile, 0, args)
    assert calls == [3], calls
    # the residual path of a tile channel reuses the tile's batch
    fd = tile.fdelta / 3
    f1 = float(tile.freqs[1])
    ch = app._predict_channel_with_beam(ms, sky['pack'], tile, 0, args, f1,
                                        fd)
    assert calls == [3], calls
    # a frequency that is no tile channel is evaluated on its own
    app._predict_channel_with_beam(ms, sky['pack'], tile, 0, args,
                                   f1 + 1234.5, fd)
    assert calls == [3, 1], calls

    # the parent path: every channel evaluates its own pattern
    monkeypatch.setattr(beams, 'element_jones_channels', real)
    cfg, t0, _ = app._beam_config(ms)
    tmjd = t0 + (np.arange(T) + 0.5) * ms.tdelta / 86400.0
    per = [beams.predict_coh_withbeam(
        sky['pack'], tile.u, tile.v, tile.w, float(f), tile.freq0, fd,
        tile.tdelta, tile.dec0, cfg, tmjd, ms.bb_tensor(), ms.Nbase, T,
        mode=dobeam - 3, coeffs='hba') for f in tile.freqs]
    ref = sum(per[1:], per[0]) / 3
    err = S.cluster_err(got, ref)
    print(f'-B {dobeam} batched vs channel by channel, per cluster:', err)
    assert max(err) <= 1e-12, err
    err = S.cluster_err(ch, per[1])
    assert max(err) <= 1e-12, err
