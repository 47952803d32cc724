"""The beamed all-channels kernels (k_predict_coh_mf_bm / _ej,
k_predict_coh_mean_bm / _ej, k_residual_mf_bm / _ej) against the fp64
per-source sandwich sum, and their wiring into
sage.calculate_residuals_multifreq and the command-line layer.

Pack, rows and channel grid are those of test_gpu_predict_channels.py: the
edge pack (clusters of 1, 64, 65 and 130 sources) with steep spectral
indices, the 135 rows of shapelet_sky.uvw_rows() (T = 3, Nbase = 45, 10
stations), and 1, NF, NF + 1 and 2 NF + 3 channels of a 200 kHz grid, NF the
larger of the two channels-per-pass constants. Gains are random in [0.2, 1],
E-Jones random complex with re/im in +-1, both different for every
(channel, timeslot, source, station).

Reference: per channel the sum over sources of g_p g_q E_p C_k E_q^H with
C_k from beams._single_source_coh in fp64, the formula of
test_gpu_element_beam._sandwich_reference (checked against it on one
channel); the single-source coherencies are computed once. For the
residual that sum goes through R.apply_jones per cluster
(sage.total_model on the CPU).

Limits. Predict: per cluster and channel max|err| / max|ref| < 1e-5, what
test_gpu_element_beam.py holds k_predict_coh_ej to and
test_gpu_predict_channels.py the unbeamed kernels. Fused residual: per
channel max|err| / max|V_ref| < 2e-5, the limit of the unbeamed fusion.
Command-line layer, GPU against CPU: 2e-4 per cluster, the limit of the
existing GPU-vs-CPU predict_coh_withbeam tests."""
import types

import numpy as np
import pytest
import torch

import channels_case as C
import shapelet_sky as S
from test_gpu_element_beam import _sandwich_reference
from test_gpu_predict_channels import count_calls, device_state, res_err
from test_gpu_predict_edges import make_edge_pack, SIZES
from sagecal_amd import beams, msdata, sky
from sagecal_amd.ops import reference as R
from sagecal_amd.ops import hip_host
from sagecal_amd.solvers import sage

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
LIMIT = 1e-5
RES_LIMIT = 2e-5
CLI_LIMIT = 2e-4
N, T = 10, 3
# gains only (_bm kernels); patterns only, one per station; both with one
# pattern per source; both with one per station (_ej kernels)
COMBOS = {'gains': (True, 0), 'ej': (False, N), 'both1': (True, 1),
          'bothN': (True, N)}


def nf():
    ext = hip_host._ext()
    return max(int(ext.PREDICT_MF_NF), int(ext.PREDICT_MF_NF_EJ))


@pytest.fixture(scope='module')
def case():
    """Pack, rows, the widest channel set, the beam buffers and the fp64
    single-source coherencies [Fmax, K, B, 2, 2], computed once."""
    NF = nf()
    Fmax = 2 * NF + 3
    grid = C.channels(Fmax, Fmax)
    pack = make_edge_pack()
    # set on the pack BEFORE any GPU call: gpu_pack caches per pack object
    pack.spec_idx[::3] = -3.0
    pack.spec_idx1[::3] = 0.4
    C.set_chunks_and_ids(pack)
    u, v, w, bb, Nbase = S.uvw_rows()
    assert (u.shape[0], Nbase, int(bb.max())) == (T * 45, 45, N - 1)
    K = pack.K
    rng = np.random.default_rng(77)
    gains = torch.tensor(rng.uniform(0.2, 1.0, (Fmax, T, K, N)),
                         dtype=torch.float32)
    E = torch.tensor(rng.uniform(-1, 1, (Fmax, T, K, N, 2, 2))
                     + 1j * rng.uniform(-1, 1, (Fmax, T, K, N, 2, 2)),
                     dtype=torch.complex64)
    src = torch.stack([torch.stack([
        beams._single_source_coh(pack, g, u, v, w, f, S.FREQ0, S.FDELTA,
                                 S.TDELTA, S.DEC0) for g in range(K)])
        for f in grid]).to(torch.complex128)
    case = dict(pack=pack, uvw=(u, v, w), bb=bb, Nbase=Nbase, NF=NF,
                Fmax=Fmax, grid=grid, gains=gains, E=E, src=src,
                uvw_d=tuple(x.to(DEV) for x in (u, v, w)),
                pairs=bb[:Nbase].to(device=DEV, dtype=torch.int32),
                refs={})
    # the vectorised sum below is _sandwich_reference's
    g1, E1 = buffers(case, 'bothN', [1])
    mine = reference(case, 'bothN', [1])[0]
    theirs = _sandwich_reference(pack, E1[0], g1[0], bb, Nbase, u, v, w,
                                 grid[1])
    assert max(S.cluster_err(mine, theirs)) < 1e-12
    return case


def subset(case, F):
    """(frequencies, their indices in the grid) of the F-channel set."""
    freqs = C.channels(F, case['Fmax'])
    return freqs, [case['grid'].index(f) for f in freqs]


def buffers(case, combo, idx):
    """(gains [F, T, K, N] or None, E [F, T, K, NE, 2, 2] or None) of the
    grid channels idx, on the CPU."""
    with_gains, NE = COMBOS[combo]
    g = case['gains'][idx].contiguous() if with_gains else None
    E = case['E'][idx][:, :, :, :NE].contiguous() if NE else None
    return g, E


def reference(case, combo, idx):
    """fp64 beamed coherencies [F, M, B, 2, 2] of the grid channels idx:
    sum over a cluster's sources of g_p g_q E_p C E_q^H."""
    key = (combo, tuple(idx))
    if key not in case['refs']:
        g, E = buffers(case, combo, idx)
        bb, Nbase = case['bb'], case['Nbase']
        t = torch.arange(bb.shape[0]) // Nbase
        p, q = bb[:, 0].long(), bb[:, 1].long()
        out = case['src'][idx]                          # [F, K, B, 2, 2]
        if E is not None:
            Ed = E.to(torch.complex128).expand(-1, -1, -1, N, -1, -1) \
                .permute(0, 2, 1, 3, 4, 5)              # [F, K, T, N, 2, 2]
            out = Ed[:, :, t, p] @ out \
                @ Ed[:, :, t, q].conj().transpose(-1, -2)
        if g is not None:
            gd = g.to(torch.float64).permute(0, 2, 1, 3)    # [F, K, T, N]
            out = (gd[:, :, t, p] * gd[:, :, t, q])[..., None, None] * out
        co = case['pack'].cluster_off.tolist()
        case['refs'][key] = torch.stack(
            [out[:, co[c]:co[c + 1]].sum(dim=1)
             for c in range(case['pack'].M)], dim=1)
    return case['refs'][key]


def dev(t):
    return None if t is None else t.to(DEV)


def gpu_channels(case, freqs, g=None, E=None, **kw):
    if g is not None or E is not None:
        kw.update(beam=dev(g), ejones=dev(E), pairs=case['pairs'],
                  Nbase=case['Nbase'])
    return hip_host.predict_coh_channels(
        case['pack'], *case['uvw_d'], freqs, S.FREQ0, S.FDELTA, S.TDELTA,
        S.DEC0, **kw)


@pytest.mark.parametrize('combo', list(COMBOS))
def test_stored_and_mean(case, combo):
    NF = case['NF']
    wide = None
    for F in (1, NF, NF + 1, 2 * NF + 3):
        freqs, idx = subset(case, F)
        g, E = buffers(case, combo, idx)
        ref = reference(case, combo, idx)
        got = gpu_channels(case, freqs, g, E)
        assert got.shape == ref.shape
        for fi in range(F):
            err = S.cluster_err(got[fi], ref[fi])
            print(f"{combo} F={F} channel {idx[fi]}, clusters of {SIZES}: "
                  + ' '.join(f'{e:.2e}' for e in err))
            assert max(err) < LIMIT, (F, fi, err)
        mean = gpu_channels(case, freqs, g, E, reduce='mean')
        err = S.cluster_err(mean, ref.mean(dim=0))
        print(f"{combo} mean of {F}: " + ' '.join(f'{e:.2e}' for e in err))
        assert mean.shape == ref.shape[1:] and max(err) < LIMIT, (F, err)
        assert torch.equal(mean, gpu_channels(case, freqs, g, E,
                                              reduce='mean'))
        wide = got
    # a channel does not depend on what shares its launch, and agrees with
    # the single-channel kernels given its rows of the buffers
    worst = 0.0
    for fi, f in enumerate(case['grid']):
        g, E = buffers(case, combo, [fi])
        alone = gpu_channels(case, [f], g, E)
        assert torch.equal(alone[0], wide[fi]), (combo, fi)
        old = hip_host.predict_coh(
            case['pack'], *case['uvw_d'], f, S.FREQ0, S.FDELTA, S.TDELTA,
            S.DEC0, beam=None if g is None else dev(g[0]),
            ejones=None if E is None else dev(E[0]), pairs=case['pairs'],
            Nbase=case['Nbase'])
        err = max(S.cluster_err(wide[fi], old))
        worst = max(worst, err)
        assert err < LIMIT, (combo, fi, err)
    print(f"{combo}: largest difference to the single-channel kernel "
          f"{worst:.2e}")


def test_identities(case):
    freqs, idx = subset(case, case['Fmax'])
    plain = gpu_channels(case, freqs)
    ones = torch.ones_like(case['gains'])
    assert torch.equal(gpu_channels(case, freqs, ones), plain)
    assert torch.equal(gpu_channels(case, freqs, ones, reduce='mean'),
                       gpu_channels(case, freqs, reduce='mean'))
    # [F, T, K, 2, 2], what element_jones_channels returns: NE = 1
    eye = torch.eye(2, dtype=torch.complex64).expand(
        len(freqs), T, case['pack'].K, 2, 2).contiguous()
    got = gpu_channels(case, freqs, None, eye)
    for fi in range(len(freqs)):
        err = S.cluster_err(got[fi], plain[fi])
        print(f"identity E, channel {fi}: "
              + ' '.join(f'{e:.2e}' for e in err))
        assert max(err) < LIMIT, (fi, err)


@pytest.fixture(scope='module')
def solved(case):
    """Hybrid-chunk state with random solutions and cluster 1 not
    subtracted, and a tile of drawn data per channel set."""
    state = C.random_state(case['pack'], N)
    assert state.nchunks == list(C.NCHUNK)
    assert case['pack'].cluster_ids[1] < 0
    tiles = {}
    for F in sorted({1, case['NF'], case['NF'] + 1, case['Fmax']}):
        freqs, _ = subset(case, F)
        tiles[F] = C.make_tile(case['uvw'], case['Nbase'], freqs)
    return dict(state=state, tiles=tiles)


def residual_reference(case, solved, combo, F, skip={1}):
    """fp64 residuals [F, B, 2, 2]: data minus the beamed coherencies of the
    subtracted clusters through R.apply_jones."""
    _, idx = subset(case, F)
    tile = solved['tiles'][F]
    cohs = reference(case, combo, idx)
    return torch.stack([
        tile.xo[fi] - sage.total_model(solved['state'], cohs[fi], case['bb'],
                                       T, case['Nbase'], skip=skip)
        for fi in range(F)])


def gpu_residuals(case, solved, F, g=None, E=None, pairs=None):
    pack, tile = case['pack'], solved['tiles'][F]
    st = device_state(solved['state'])
    td = C.to_device(tile, DEV)
    return hip_host.residuals_multifreq(
        pack, td.xo, td.u, td.v, td.w, tile.freqs, S.FREQ0, S.FDELTA,
        S.TDELTA, S.DEC0, st.J, sage._chunk_table(st, T, case['Nbase'], DEV),
        case['pairs'] if pairs is None else pairs,
        subtract=torch.tensor([c >= 0 for c in pack.cluster_ids],
                              device=DEV),
        beam=dev(g), ejones=dev(E))


@pytest.mark.parametrize('combo', ['gains', 'bothN'])
def test_fused_beamed_residual(case, solved, combo):
    for F, tile in solved['tiles'].items():
        _, idx = subset(case, F)
        g, E = buffers(case, combo, idx)
        got = gpu_residuals(case, solved, F, g, E)
        ref = residual_reference(case, solved, combo, F)
        V = tile.xo - ref
        err = res_err(got, ref, V)
        print(f"{combo} fused residual F={F}: "
              + ' '.join(f'{e:.2e}' for e in err))
        assert got.shape == ref.shape and max(err) < RES_LIMIT, (F, err)
        # with cluster 1 left in the answer would be far outside the limit
        miss = res_err(got, residual_reference(case, solved, combo, F,
                                               skip=set()), V)
        assert min(miss) > 100 * RES_LIMIT, (F, miss)
        # and so would it be with the beam ignored
        nobeam = res_err(gpu_residuals(case, solved, F), ref, V)
        assert min(nobeam) > 100 * RES_LIMIT, (F, nobeam)


@pytest.mark.parametrize('combo,col', [('gains', 0), ('bothN', 1)])
def test_negative_pair_keeps_the_data(case, solved, combo, col):
    F, Nbase = case['Fmax'], case['Nbase']
    tile = solved['tiles'][F]
    _, idx = subset(case, F)
    g, E = buffers(case, combo, idx)
    pairs = case['pairs'].clone()
    pairs[11, col] = -1
    got = gpu_residuals(case, solved, F, g, E, pairs=pairs).cpu()
    hit = torch.arange(T) * Nbase + 11
    assert torch.equal(got[:, hit], tile.xo[:, hit].to(torch.complex64))
    keep = torch.ones(T * Nbase, dtype=torch.bool)
    keep[hit] = False
    ref = residual_reference(case, solved, combo, F)
    err = res_err(got[:, keep], ref[:, keep], (tile.xo - ref)[:, keep])
    print(f"{combo}, negative pair, other rows: "
          + ' '.join(f'{e:.2e}' for e in err))
    assert max(err) < RES_LIMIT, err
    # the predict entries have no row to keep: they refuse the table
    with pytest.raises(ValueError):
        hip_host.predict_coh_channels(
            case['pack'], *case['uvw_d'], tile.freqs, S.FREQ0, S.FDELTA,
            S.TDELTA, S.DEC0, beam=dev(g), ejones=dev(E), pairs=pairs,
            Nbase=Nbase)


def test_sage_takes_the_fused_beamed_path(case, solved, monkeypatch):
    pack, bbd, F = case['pack'], case['bb'].to(DEV), case['Fmax']
    tile = solved['tiles'][F]
    td = C.to_device(tile, DEV)
    _, idx = subset(case, F)
    g, E = (dev(b) for b in buffers(case, 'bothN', idx))

    def coh_fn(f):
        fi = tile.freqs.index(f)
        return hip_host.predict_coh(
            pack, td.u, td.v, td.w, f, S.FREQ0, S.FDELTA, S.TDELTA, S.DEC0,
            beam=g[fi], ejones=E[fi], pairs=case['pairs'],
            Nbase=case['Nbase'])
    n = count_calls(monkeypatch)
    beam = dict(beam=g, ejones=E)
    got = sage.calculate_residuals_multifreq(
        device_state(solved['state']), pack, td, bbd, coh_fn=coh_fn,
        beam=beam)
    assert (n['residuals_multifreq'].calls, n['predict_coh'].calls) == (1, 0)
    monkeypatch.setenv('SAGECAL_RESIDUAL_LOOP', '1')
    loop = sage.calculate_residuals_multifreq(
        device_state(solved['state']), pack, td, bbd, coh_fn=coh_fn,
        beam=beam)
    assert (n['residuals_multifreq'].calls, n['predict_coh'].calls) == (1, F)
    ref = residual_reference(case, solved, 'bothN', F)
    V = tile.xo - ref
    for name, r in (('fused', got), ('loop', loop)):
        err = res_err(r, ref, V)
        print(f"sage beamed residuals, {name}: "
              + ' '.join(f'{e:.2e}' for e in err))
        assert max(err) < RES_LIMIT, (name, err)
    err = res_err(got, loop.cpu().to(torch.complex128), V)
    assert max(err) < RES_LIMIT, err


@pytest.fixture(scope='module')
def observation(tmp_path_factory):
    """Shapelet-free pack and two 3-channel NpzMS files with element
    layouts, single-stage and two-stage (tile_enu)."""
    d = tmp_path_factory.mktemp('beamms')
    srcs, clist = sky.make_synthetic_sky(M=3, nsrc_per_cluster=3, seed=1)
    pack = R.SourcePack(sky.build_clusters(srcs, clist, 0.0, np.pi / 4,
                                           150e6))
    rng = np.random.default_rng(3)
    keys = dict(element_enu=rng.uniform(-20, 20, (8, 12, 3)), lon=0.1,
                lat=0.92, tmjd0=57000.0)
    grid = (np.arange(4) - 1.5) * 1.25
    gx, gy = np.meshgrid(grid, grid)
    dip = np.stack([np.column_stack([gx.ravel(), gy.ravel(), np.zeros(16)])
                    + rng.uniform(-0.05, 0.05, (16, 3)) for _ in range(8)])
    files = {}
    for name, extra in (('single', {}),
                        ('tile', dict(tile_enu=dip, tile_ra0=0.02,
                                      tile_dec0=np.pi / 4 - 0.014))):
        msf = str(d / f'{name}.npz')
        msdata.make_synthetic_npz(msf, N=8, tilesz=4, Ntime=4, Nchan=3,
                                  pack=pack, bandwidth=600e3,
                                  noise_sigma=1e-3, seed=5, ra0=0.0,
                                  dec0=np.pi / 4)
        z = dict(np.load(msf))
        z.update(keys, **extra)
        np.savez(msf, **z)
        files[name] = msf
    return pack, files


@pytest.mark.parametrize('stage', ['single', 'tile'])
@pytest.mark.parametrize('dobeam', [4, 5, 6])
def test_cli_wideband_predict_is_one_launch(observation, monkeypatch,
                                            dobeam, stage):
    from sagecal_amd.apps import sagecal as app
    pack, files = observation
    args = types.SimpleNamespace(dobeam=dobeam, elem_type='hba')
    out = {}
    n = count_calls(monkeypatch)
    for where in ('cpu', DEV):
        ms = msdata.NpzMS(files[stage], tilesz=4, device=where)
        tile = ms.load_tile(0)
        assert len(tile.freqs) == 3
        out[where] = app._predict_with_beam(ms, pack, tile, 0, args)
    assert (n['predict_coh_channels'].calls, n['predict_coh'].calls) == (1, 0)
    assert out[DEV].is_cuda and bool(out['cpu'].abs().max() > 0)
    err = S.cluster_err(out[DEV], out['cpu'])
    print(f"-B {dobeam} {stage}-stage, gpu vs cpu, per cluster: "
          + ' '.join(f'{e:.2e}' for e in err))
    assert max(err) < CLI_LIMIT, err


def test_errors_and_empty(case, monkeypatch):
    freqs, idx = subset(case, 2)
    g, E = buffers(case, 'bothN', idx)
    with pytest.raises(ValueError):               # wrong leading F
        gpu_channels(case, freqs, case['gains'][:3].contiguous())
    with pytest.raises(ValueError):
        gpu_channels(case, freqs, None, case['E'][:3].contiguous())
    with pytest.raises(ValueError):               # pairs outside Nsta
        gpu_channels(case, freqs, g[..., :N - 1].contiguous())
    with pytest.raises(ValueError):               # NE = 2
        gpu_channels(case, freqs, g, E[:, :, :, :2].contiguous())
    with pytest.raises(ValueError):               # fewer sources than K
        gpu_channels(case, freqs, g[:, :, :-1].contiguous())
    with pytest.raises(ValueError):               # no pairs
        hip_host.predict_coh_channels(
            case['pack'], *case['uvw_d'], freqs, S.FREQ0, S.FDELTA, S.TDELTA,
            S.DEC0, beam=dev(g))
    spack, _ = S.make_pack()
    sg = torch.ones(2, T, spack.K, N)
    with pytest.raises(ValueError):               # shapelet pack
        hip_host.predict_coh_channels(
            spack, *case['uvw_d'], freqs, S.FREQ0, S.FDELTA, S.TDELTA,
            S.DEC0, beam=sg.to(DEV), pairs=case['pairs'],
            Nbase=case['Nbase'])
    n = count_calls(monkeypatch)
    out = gpu_channels(case, [], case['gains'][:0], case['E'][:0])
    assert out.shape == (0, len(SIZES), T * 45, 2, 2) and out.is_cuda
    assert n['predict_coh_channels'].calls == 0
