"""The all-channels kernels k_predict_coh_mf, k_predict_coh_mean and
k_residual_mf against the fp64 reference, and their wiring into
sage.calculate_residuals_multifreq and sage.precalc_coherencies.

Pack: test_gpu_predict_edges.make_edge_pack() (clusters of 1, 64, 65 and
130 sources, all four source types in second-tile slots, negative and
polarised fluxes) with steep spectral indices on every third source. Rows:
the 135 of shapelet_sky.uvw_rows() (one full 128-thread block and a 7-row
tail), its first row alone, and the 135 stretched to |uvw| = 3e-3 s.
Channels: 1, NF, NF + 1 and 2 NF + 3 of a 200 kHz grid around FREQ0 that
holds FREQ0 itself, NF the channels a thread carries per pass.

Limits. Predict: per cluster and channel max|err| / max|ref| < 1e-5, the
limit test_gpu_predict_edges.py holds k_predict_coh to. Fused residual: per
channel max|err| / max|V_ref| < 2e-5 with V_ref the subtracted model, the
sum, rounded up, of that 1e-5 and the 5e-6 of
test_gpu.py::test_apply_jones_and_cost for the two kernels it fuses."""
import pytest
import torch

import channels_case as C
import shapelet_sky as S
from test_gpu_predict_edges import make_edge_pack, SIZES
from sagecal_amd.ops import reference as R
from sagecal_amd.ops import hip_host
from sagecal_amd.solvers import sage

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
LIMIT = 1e-5
RES_LIMIT = 2e-5
N = 10
ROWSETS = ('all135', 'first1', 'long')


def nf():
    return int(hip_host._ext().PREDICT_MF_NF)


@pytest.fixture(scope='module')
def case():
    """Pack, row sets, the widest channel set and its fp64 reference per
    (row set, channel), computed once; every narrower set is a slice."""
    NF = nf()
    Fmax = 2 * NF + 3
    grid = C.channels(Fmax, Fmax)
    pack = make_edge_pack()
    # set on the pack BEFORE any GPU call: gpu_pack caches per pack object
    pack.spec_idx[::3] = -3.0
    pack.spec_idx1[::3] = 0.4
    C.set_chunks_and_ids(pack)
    sel = slice(0, pack.K)
    scaled = R._source_flux_at(pack, sel, grid[0], S.FREQ0)[0]
    assert float(((scaled - pack.sI) / pack.sI).abs().max()) > 0.01
    assert S.FREQ0 in grid

    u, v, w, bb, Nbase = S.uvw_rows()
    uvw = torch.stack([u, v, w])
    k = 3e-3 / float(uvw.abs().max())
    rowsets = {'all135': uvw, 'first1': uvw[:, :1].contiguous(),
               'long': uvw * k}
    refs = {n: torch.stack([R.predict_coh(pack, *rs, f, S.FREQ0, S.FDELTA,
                                          S.TDELTA, S.DEC0) for f in grid])
            for n, rs in rowsets.items()}
    return dict(pack=pack, rowsets=rowsets, refs=refs, grid=grid, bb=bb,
                Nbase=Nbase, NF=NF, Fmax=Fmax)


def subset(case, F):
    """(frequencies, their indices in the grid) of the F-channel set."""
    freqs = C.channels(F, case['Fmax'])
    return freqs, [case['grid'].index(f) for f in freqs]


def gpu_channels(case, rows, freqs, **kw):
    u, v, w = (t.to(DEV) for t in case['rowsets'][rows])
    return hip_host.predict_coh_channels(case['pack'], u, v, w, freqs,
                                         S.FREQ0, S.FDELTA, S.TDELTA,
                                         S.DEC0, **kw)


@pytest.mark.parametrize('rows', ROWSETS)
def test_all_channels_stored(case, rows):
    NF = case['NF']
    worst_old = 0.0
    wide = None
    for F in (1, NF, NF + 1, 2 * NF + 3):
        freqs, idx = subset(case, F)
        got = gpu_channels(case, rows, freqs)
        ref = case['refs'][rows][idx]
        assert got.shape == ref.shape
        for fi in range(F):
            err = S.cluster_err(got[fi], ref[fi])
            print(f"{rows} F={F} channel {idx[fi]}, clusters of {SIZES}: "
                  + ' '.join(f'{e:.2e}' for e in err))
            assert max(err) < LIMIT, (F, fi, err)
        wide = got
    # a channel does not depend on what shares its launch, and agrees with
    # the single-channel kernel
    u, v, w = (t.to(DEV) for t in case['rowsets'][rows])
    for fi, f in enumerate(case['grid']):
        alone = gpu_channels(case, rows, [f])
        assert torch.equal(alone[0], wide[fi]), (rows, fi)
        old = hip_host.predict_coh(case['pack'], u, v, w, f, S.FREQ0,
                                   S.FDELTA, S.TDELTA, S.DEC0)
        err = max(S.cluster_err(wide[fi], old))
        worst_old = max(worst_old, err)
        assert err < LIMIT, (rows, fi, err)
    print(f"{rows}: largest difference to k_predict_coh {worst_old:.2e}")


@pytest.mark.parametrize('rows', ROWSETS)
def test_channel_mean(case, rows):
    NF = case['NF']
    for F in (1, NF, NF + 1, 2 * NF + 3):
        freqs, idx = subset(case, F)
        got = gpu_channels(case, rows, freqs, reduce='mean')
        ref = case['refs'][rows][idx].mean(dim=0)
        assert got.shape == ref.shape
        err = S.cluster_err(got, ref)
        print(f"{rows} mean of {F}: " + ' '.join(f'{e:.2e}' for e in err))
        assert max(err) < LIMIT, (F, err)
        again = gpu_channels(case, rows, freqs, reduce='mean')
        assert torch.equal(got, again)


def res_err(got, ref, V):
    """max|got - ref| / max|V| per channel."""
    got = got.detach().cpu().to(torch.complex128)
    F = ref.shape[0]
    num = (got - ref).abs().reshape(F, -1).max(dim=1).values
    den = V.abs().reshape(F, -1).max(dim=1).values
    return [float(n / d) for n, d in zip(num, den)]


@pytest.fixture(scope='module')
def solved(case):
    """Hybrid-chunk state with random solutions and cluster 1 not
    subtracted; the fp64 CPU residuals of every channel set, and those with
    cluster 1 subtracted as well."""
    pack, bb, Nbase = case['pack'], case['bb'], case['Nbase']
    state = C.random_state(pack, N)
    assert state.nchunks == list(C.NCHUNK) and pack.cluster_ids[1] < 0
    assert sage._chunk_table(state, 3, Nbase, 'cpu').tolist() == \
        [[0, 0, 0], [1, 1, 2], [3, 4, 5], [6, 6, 6]]
    out = dict(state=state, tiles={}, refs={}, refs_all={})
    for F in sorted({1, case['NF'], case['NF'] + 1, case['Fmax']}):
        freqs, _ = subset(case, F)
        tile = C.make_tile(case['rowsets']['all135'], Nbase, freqs)
        out['tiles'][F] = tile
        out['refs'][F] = sage.calculate_residuals_multifreq(state, pack,
                                                            tile, bb)
        ids = pack.cluster_ids
        pack.cluster_ids = list(range(pack.M))
        try:
            out['refs_all'][F] = sage.calculate_residuals_multifreq(
                state, pack, tile, bb)
        finally:
            pack.cluster_ids = ids
    return out


def device_state(state):
    st = sage.CalState.__new__(sage.CalState)
    st.__dict__.update({k: v for k, v in state.__dict__.items()
                        if not k.startswith('_')})
    st.J = state.J.to(device=DEV, dtype=torch.complex64)
    return st


def test_fused_residual(case, solved):
    pack, bb, Nbase = case['pack'], case['bb'], case['Nbase']
    st = device_state(solved['state'])
    pairs = bb[:Nbase].to(device=DEV, dtype=torch.int32)
    tab = sage._chunk_table(st, 3, Nbase, DEV)
    subtract = torch.tensor([c >= 0 for c in pack.cluster_ids], device=DEV)
    for F, tile in solved['tiles'].items():
        td = C.to_device(tile, DEV)
        got = hip_host.residuals_multifreq(
            pack, td.xo, td.u, td.v, td.w, tile.freqs, S.FREQ0, S.FDELTA,
            S.TDELTA, S.DEC0, st.J, tab, pairs, subtract=subtract)
        ref = solved['refs'][F]
        V = tile.xo - ref
        err = res_err(got, ref, V)
        print(f"fused residual F={F}: " + ' '.join(f'{e:.2e}' for e in err))
        assert got.shape == ref.shape and max(err) < RES_LIMIT, (F, err)
        # with cluster 1 left in the answer would be far outside the limit
        miss = res_err(got, solved['refs_all'][F], V)
        assert min(miss) > 100 * RES_LIMIT, (F, miss)


def test_negative_pair_keeps_the_data(case, solved, monkeypatch):
    pack, Nbase, F = case['pack'], case['Nbase'], case['Fmax']
    tile = solved['tiles'][F]
    td = C.to_device(tile, DEV)
    bbd = case['bb'].clone()
    hit = torch.arange(3) * Nbase + 11
    bbd[hit, 0] = -1
    bbd = bbd.to(DEV)
    got = sage.calculate_residuals_multifreq(
        device_state(solved['state']), pack, td, bbd)
    assert torch.equal(got[:, hit.to(DEV)], td.xo[:, hit.to(DEV)])
    monkeypatch.setenv('SAGECAL_RESIDUAL_LOOP', '1')
    loop = sage.calculate_residuals_multifreq(
        device_state(solved['state']), pack, td, bbd)
    keep = torch.ones(3 * Nbase, dtype=torch.bool)
    keep[hit] = False
    V = (tile.xo - solved['refs'][F])[:, keep]
    err = res_err(got[:, keep.to(DEV)],
                  loop[:, keep.to(DEV)].cpu().to(torch.complex128), V)
    print("negative pair, fused against loop: "
          + ' '.join(f'{e:.2e}' for e in err))
    assert max(err) < RES_LIMIT, err


class Counter:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a, **k):
        self.calls += 1
        return self.fn(*a, **k)


def count_calls(monkeypatch):
    ext = hip_host._ext()
    counters = {}
    for name in ('residuals_multifreq', 'predict_coh_channels',
                 'predict_coh'):
        counters[name] = Counter(getattr(ext, name))
        monkeypatch.setattr(ext, name, counters[name])
    return counters


def test_sage_takes_the_fused_path(case, solved, monkeypatch):
    pack, bbd, F = case['pack'], case['bb'].to(DEV), case['Fmax']
    tile = solved['tiles'][F]
    td = C.to_device(tile, DEV)
    n = count_calls(monkeypatch)
    got = sage.calculate_residuals_multifreq(
        device_state(solved['state']), pack, td, bbd)
    assert (n['residuals_multifreq'].calls, n['predict_coh'].calls) == (1, 0)
    mean = sage.precalc_coherencies(pack, td)
    assert (n['predict_coh_channels'].calls, n['predict_coh'].calls) == (1, 0)

    monkeypatch.setenv('SAGECAL_RESIDUAL_LOOP', '1')
    loop = sage.calculate_residuals_multifreq(
        device_state(solved['state']), pack, td, bbd)
    mean_loop = sage.precalc_coherencies(pack, td)
    assert n['predict_coh'].calls == 2 * F
    assert (n['residuals_multifreq'].calls,
            n['predict_coh_channels'].calls) == (1, 1)
    ref = solved['refs'][F]
    V = tile.xo - ref
    for name, r in (('fused', got), ('loop', loop)):
        err = res_err(r, ref, V)
        print(f"sage residuals, {name}: " + ' '.join(f'{e:.2e}' for e in err))
        assert max(err) < RES_LIMIT, (name, err)
    mref = case['refs']['all135'].mean(dim=0)
    for name, m in (('fused', mean), ('loop', mean_loop)):
        err = S.cluster_err(m, mref)
        print(f"precalc mean, {name}: " + ' '.join(f'{e:.2e}' for e in err))
        assert max(err) < LIMIT, (name, err)


def test_shapelets_and_coh_fn_take_the_loop(case, solved, monkeypatch):
    F = case['NF'] + 1
    n = count_calls(monkeypatch)
    fused = lambda: (n['residuals_multifreq'].calls
                     + n['predict_coh_channels'].calls)
    bbd = case['bb'].to(DEV)

    # shapelet pack: the loop, with the values the switch gives
    spack, _ = S.make_pack()
    tile = C.make_tile(case['rowsets']['all135'], case['Nbase'],
                       solved['tiles'][F].freqs)
    td = C.to_device(tile, DEV)
    st = C.random_state(spack, N, device=DEV, dtype=torch.complex64)
    res = sage.calculate_residuals_multifreq(st, spack, td, bbd)
    mean = sage.precalc_coherencies(spack, td)
    assert fused() == 0 and n['predict_coh'].calls == 2 * F
    monkeypatch.setenv('SAGECAL_RESIDUAL_LOOP', '1')
    assert torch.equal(res, sage.calculate_residuals_multifreq(
        st, spack, td, bbd))
    assert torch.equal(mean, sage.precalc_coherencies(spack, td))
    monkeypatch.delenv('SAGECAL_RESIDUAL_LOOP')

    # coh_fn: the loop, on a pack the fused path would take
    pack = case['pack']
    std = device_state(solved['state'])
    coh_fn = lambda f: hip_host.predict_coh(
        pack, td.u, td.v, td.w, f, S.FREQ0, S.FDELTA, S.TDELTA, S.DEC0)
    res = sage.calculate_residuals_multifreq(std, pack, td, bbd,
                                             coh_fn=coh_fn)
    assert fused() == 0
    monkeypatch.setenv('SAGECAL_RESIDUAL_LOOP', '1')
    assert torch.equal(res, sage.calculate_residuals_multifreq(
        std, pack, td, bbd))


def test_errors_and_empty(case):
    spack, _ = S.make_pack()
    u, v, w = (t.to(DEV) for t in case['rowsets']['all135'])
    with pytest.raises(ValueError):
        hip_host.predict_coh_channels(spack, u, v, w, [S.FREQ0], S.FREQ0,
                                      S.FDELTA, S.TDELTA, S.DEC0)
    out = gpu_channels(case, 'all135', [])
    assert out.shape == (0, len(SIZES), 135, 2, 2)
    assert out.dtype == torch.complex64 and out.is_cuda
    none = hip_host.predict_coh_channels(
        case['pack'], u[:0], v[:0], w[:0], [S.FREQ0], S.FREQ0, S.FDELTA,
        S.TDELTA, S.DEC0)
    assert none.shape == (1, len(SIZES), 0, 2, 2)
