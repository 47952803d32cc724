"""The all-channels shapelet kernels (k_shapelet_coh_mf, k_shapelet_coh_mean,
k_shapelet_residual_mf and their _bm / _ej variants) behind shapelets=True,
against fp64 references, and their wiring into sage behind
SAGECAL_SHAPELET_CHANNELS=1.

Packs: shapelet_sky.make_pack() (cluster 0: n0 = 1 and n0 = 5 with
projection; cluster 1: no entry; cluster 2: last source n0 = 12) and the
one-source pack of test_cluster_of_one_shapelet, steep spectral indices on
the shapelet sources. Rows: the 135 of uvw_rows() (a full block and a 7-row
tail) and the first alone. Channels: 1, NF, NF + 1 and 2 NF + 3 of the
200 kHz grid of channels_case, NF the exported constant of the variant.
Variants: no beam, gains [F, T, K, 10] in [0.2, 1], patterns
[F, T, K, NE, 2, 2] with re/im in +-1 for NE = 1 and NE = 10, and gains
with either.

References, all fp64 on the CPU: reference.predict_coh per channel (plain),
shapelet_sky.beamed_reference (gains), dispatch._beamed_coh_reference
(NE = 1) and the per-source sandwich sum of test_gpu_beam_channels
(NE = 10). Limits: per cluster and channel max|err| / max|ref| < 1e-5, what
test_gpu_shapelet_kernel.py holds k_shapelet_coh to and
test_gpu_beam_channels.py the _bm and _ej kernels; fused residual per
channel max|err| / max|V_ref| < 2e-5, as in test_gpu_predict_channels.py."""
import numpy as np
import pytest
import torch

import channels_case as C
import shapelet_sky as S
from test_gpu_beam_channels import reference as sandwich_reference
from test_gpu_predict_channels import count_calls, device_state, res_err
from sagecal_amd import beams
from sagecal_amd.ops import dispatch, hip_host
from sagecal_amd.ops import reference as R
from sagecal_amd.solvers import sage

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
LIMIT = 1e-5
RES_LIMIT = 2e-5
N, T = 10, 3
SPECS = {'standard': dict(),
         'one': dict(spec=((0, 0, 5, 1.5e-3, True, 0.8, 1.3, 0.4),), M=2,
                     nsrc=1)}
# (with gains, patterns per source)
VARIANTS = {'plain': (False, 0), 'gains': (True, 0), 'ej1': (False, 1),
            'ejN': (False, N), 'both1': (True, 1), 'bothN': (True, N)}
ARGS = (S.FREQ0, S.FDELTA, S.TDELTA, S.DEC0)


def nf(variant):
    ext = hip_host._ext()
    return int(ext.SHAPELET_MF_NF_EJ if VARIANTS[variant][1]
               else ext.SHAPELET_MF_NF)


@pytest.fixture(scope='module')
def cases():
    """Per pack: the pack, its twin without shapelet sources, rows, the
    widest channel grid, beam buffers and the fp64 single-source
    coherencies [Fmax, K, B, 2, 2]; references are computed once per
    (variant, channel) and kept in 'refs'."""
    Fmax = 2 * max(nf('plain'), nf('ejN')) + 3
    grid = C.channels(Fmax, Fmax)
    u, v, w, bb, Nbase = S.uvw_rows()
    out = {}
    for name, kw in SPECS.items():
        pack, gis = S.make_pack(**kw)
        # set on the pack BEFORE any GPU call: gpu_pack caches per pack
        pack.spec_idx[gis] = -3.0
        pack.spec_idx1[gis] = 0.4
        lo = R._source_flux_at(pack, slice(0, pack.K), grid[0], S.FREQ0)[0]
        hi = R._source_flux_at(pack, slice(0, pack.K), grid[-1], S.FREQ0)[0]
        assert float(((lo - hi) / hi)[gis].abs().min()) > 0.01
        rng = np.random.default_rng(77)
        shape = (Fmax, T, pack.K, N)
        out[name] = dict(
            pack=pack, gis=gis, plain=S.make_pack(**dict(kw, spec=()))[0],
            uvw=(u, v, w), bb=bb, Nbase=Nbase, grid=grid, Fmax=Fmax, refs={},
            gains=torch.tensor(rng.uniform(0.2, 1.0, shape),
                               dtype=torch.float32),
            E=torch.tensor(rng.uniform(-1, 1, shape + (2, 2))
                           + 1j * rng.uniform(-1, 1, shape + (2, 2)),
                           dtype=torch.complex64),
            src=torch.stack([torch.stack([
                beams._single_source_coh(pack, g, u, v, w, f, *ARGS)
                for g in range(pack.K)]) for f in grid]))
    C.set_chunks_and_ids(out['standard']['pack'], nchunk=(1, 2, 3),
                         negative=0)
    return out


def reference(case, variant, idx):
    """fp64 coherencies [F, M, B, 2, 2] of the grid channels idx."""
    gains, NE = VARIANTS[variant]
    if NE == N:
        return sandwich_reference(case, 'bothN' if gains else 'ej', idx)
    pack, uvw, bb, Nbase = (case[k] for k in ('pack', 'uvw', 'bb', 'Nbase'))
    for fi in idx:
        if (variant, fi) in case['refs']:
            continue
        f = case['grid'][fi]
        if NE:
            ref = dispatch._beamed_coh_reference(
                pack, *uvw, fi, f, *ARGS, case['gains'] if gains else None,
                case['E'][:, :, :, :1], bb[:Nbase], Nbase)
        elif gains:
            ref = S.beamed_reference(pack, range(pack.K), case['gains'][fi],
                                     bb, Nbase, *uvw, f)
        else:
            ref = R.predict_coh(pack, *uvw, f, *ARGS)
        case['refs'][variant, fi] = ref
    return torch.stack([case['refs'][variant, fi] for fi in idx])


def beam_kw(case, variant, idx, nrow=T * 45):
    """beam, ejones, pairs and Nbase of the grid channels idx for the first
    nrow rows (whole timeslots, or the first row alone)."""
    gains, NE = VARIANTS[variant]
    if not gains and not NE:
        return {}
    Nbase = min(nrow, case['Nbase'])
    nt = nrow // Nbase
    kw = dict(pairs=case['bb'][:Nbase].to(device=DEV, dtype=torch.int32),
              Nbase=Nbase)
    if gains:
        kw['beam'] = case['gains'][idx][:, :nt].contiguous().to(DEV)
    if NE:
        kw['ejones'] = case['E'][idx][:, :nt, :, :NE].contiguous().to(DEV)
    return kw


def subset(case, F):
    freqs = C.channels(F, case['Fmax'])
    return freqs, [case['grid'].index(f) for f in freqs]


def gpu_channels(case, variant, F, nrow=T * 45, pack=None, **kw):
    freqs, idx = subset(case, F)
    u, v, w = (t[:nrow].to(DEV) for t in case['uvw'])
    return hip_host.predict_coh_channels(
        pack or case['pack'], u, v, w, freqs, *ARGS,
        **beam_kw(case, variant, idx, nrow), **kw)


@pytest.mark.parametrize('nrow', [T * 45, 1])
@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('name', list(SPECS))
def test_stored_and_mean(cases, name, variant, nrow):
    case, NF = cases[name], nf(variant)
    for F in (1, NF, NF + 1, 2 * NF + 3):
        _, idx = subset(case, F)
        ref = reference(case, variant, idx)[:, :, :nrow]
        got = gpu_channels(case, variant, F, nrow, shapelets=True)
        assert got.shape == ref.shape
        for fi in range(F):
            err = S.cluster_err(got[fi], ref[fi])
            print(f"{name} {variant} rows={nrow} F={F} channel {idx[fi]}: "
                  + ' '.join(f'{e:.2e}' for e in err))
            assert max(err) < LIMIT, (F, fi, err)
        mean = gpu_channels(case, variant, F, nrow, shapelets=True,
                            reduce='mean')
        err = S.cluster_err(mean, ref.mean(dim=0))
        print(f"{name} {variant} rows={nrow} mean of {F}: "
              + ' '.join(f'{e:.2e}' for e in err))
        assert mean.shape == ref.shape[1:] and max(err) < LIMIT, (F, err)
        assert torch.equal(mean, gpu_channels(
            case, variant, F, nrow, shapelets=True, reduce='mean'))
    # `got` is the widest launch: a channel does not depend on what shares
    # its launch
    u, v, w = (t[:nrow].to(DEV) for t in case['uvw'])
    for k, fi in enumerate(idx):
        alone = hip_host.predict_coh_channels(
            case['pack'], u, v, w, [case['grid'][fi]], *ARGS, shapelets=True,
            **beam_kw(case, variant, [fi], nrow))
        assert torch.equal(alone[0], got[k]), (variant, fi)
    # cluster 1 has no shapelet source: the main kernel's result, untouched
    main = gpu_channels(case, variant, F, nrow, pack=case['plain'])
    assert torch.equal(got[:, 1], main[:, 1])
    # and without shapelet sources shapelets=True is the plain call
    assert torch.equal(main, gpu_channels(case, variant, F, nrow,
                                          pack=case['plain'], shapelets=True))


@pytest.fixture(scope='module')
def solved(cases):
    """Hybrid-chunk state with random solutions and a tile of drawn data
    per channel count; shapelet cluster 0 is solved but not subtracted."""
    case = cases['standard']
    state = C.random_state(case['pack'], N)
    assert state.nchunks == [1, 2, 3] and case['pack'].cluster_ids[0] < 0
    tiles = {F: C.make_tile(case['uvw'], case['Nbase'], subset(case, F)[0])
             for F in {1, case['Fmax']} | {nf(v) + d for v in VARIANTS
                                           for d in (0, 1)}
             | {2 * nf(v) + 3 for v in VARIANTS}}
    return dict(state=state, tiles=tiles)


def cpu_residuals(case, solved, variant, F, ids=None):
    """sage.calculate_residuals_multifreq in fp64 on the CPU over the
    variant's reference coherencies."""
    pack, tile = case['pack'], solved['tiles'][F]
    coh_fn = lambda f: reference(case, variant, [case['grid'].index(f)])[0]
    keep, pack.cluster_ids = pack.cluster_ids, ids or pack.cluster_ids
    try:
        return sage.calculate_residuals_multifreq(
            solved['state'], pack, tile, case['bb'], coh_fn=coh_fn)
    finally:
        pack.cluster_ids = keep


def gpu_residuals(case, solved, variant, F, pairs=None, pack=None, **kw):
    tile = solved['tiles'][F]
    st, td = device_state(solved['state']), C.to_device(tile, DEV)
    bm = {k: t for k, t in beam_kw(case, variant, subset(case, F)[1]).items()
          if k in ('beam', 'ejones')}
    if pairs is None:
        pairs = case['bb'][:45].to(device=DEV, dtype=torch.int32)
    ids = case['pack'].cluster_ids
    return hip_host.residuals_multifreq(
        pack or case['pack'], td.xo, td.u, td.v, td.w, tile.freqs, *ARGS,
        st.J, sage._chunk_table(st, T, 45, DEV), pairs,
        subtract=torch.tensor([c >= 0 for c in ids]), **bm, **kw)


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_fused_residual(cases, solved, variant):
    case, NF = cases['standard'], nf(variant)
    for F in (1, NF, NF + 1, 2 * NF + 3):
        tile = solved['tiles'][F]
        got = gpu_residuals(case, solved, variant, F, shapelets=True)
        ref = cpu_residuals(case, solved, variant, F)
        V = tile.xo - ref
        err = res_err(got, ref, V)
        print(f"{variant} fused residual F={F}: "
              + ' '.join(f'{e:.2e}' for e in err))
        assert got.shape == ref.shape and max(err) < RES_LIMIT, (F, err)
        # with cluster 0 subtracted the answer would be far outside
        miss = res_err(got, cpu_residuals(case, solved, variant, F,
                                          ids=[0, 1, 2]), V)
        assert min(miss) > 100 * RES_LIMIT, (F, miss)
    # a row with a negative pair entry keeps the data
    pairs = case['bb'][:45].to(device=DEV, dtype=torch.int32)
    pairs[11, 1] = -1
    hit = torch.arange(T) * 45 + 11
    got = gpu_residuals(case, solved, variant, F, pairs=pairs,
                        shapelets=True).cpu()
    assert torch.equal(got[:, hit], tile.xo[:, hit].to(torch.complex64))
    keep = torch.ones(T * 45, dtype=torch.bool)
    keep[hit] = False
    err = res_err(got[:, keep], ref[:, keep], V[:, keep])
    assert max(err) < RES_LIMIT, err
    # without shapelet sources shapelets=True is the plain call
    plain = gpu_residuals(case, solved, variant, F, pack=case['plain'])
    assert torch.equal(plain, gpu_residuals(
        case, solved, variant, F, pack=case['plain'], shapelets=True))


def test_sage_takes_the_shapelet_path(cases, solved, monkeypatch):
    case = cases['standard']
    pack, bbd, F = case['pack'], case['bb'].to(DEV), case['Fmax']
    tile = solved['tiles'][F]
    td = C.to_device(tile, DEV)
    st = device_state(solved['state'])
    n = count_calls(monkeypatch)
    monkeypatch.setenv('SAGECAL_SHAPELET_CHANNELS', '1')
    got = sage.calculate_residuals_multifreq(st, pack, td, bbd)
    assert (n['residuals_multifreq'].calls, n['predict_coh'].calls) == (1, 0)
    mean = sage.precalc_coherencies(pack, td)
    assert (n['predict_coh_channels'].calls, n['predict_coh'].calls) == (1, 0)
    monkeypatch.setenv('SAGECAL_RESIDUAL_LOOP', '1')
    loop = sage.calculate_residuals_multifreq(st, pack, td, bbd)
    mean_loop = sage.precalc_coherencies(pack, td)
    assert n['predict_coh'].calls == 2 * F
    assert (n['residuals_multifreq'].calls,
            n['predict_coh_channels'].calls) == (1, 1)
    ref = cpu_residuals(case, solved, 'plain', F)
    mref = reference(case, 'plain', list(range(F))).mean(dim=0)
    for name, r, m in (('fused', got, mean), ('loop', loop, mean_loop)):
        err = res_err(r, ref, tile.xo - ref)
        merr = S.cluster_err(m, mref)
        print(f"sage, {name}: residuals " + ' '.join(f'{e:.2e}' for e in err)
              + ', mean ' + ' '.join(f'{e:.2e}' for e in merr))
        assert max(err) < RES_LIMIT and max(merr) < LIMIT, (name, err, merr)
