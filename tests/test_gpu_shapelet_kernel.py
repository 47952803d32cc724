"""k_shapelet_coh on the GPU: the shapelet sources of a pack evaluated by
the HIP kernel from the device-resident table, against the fp64 reference,
the torch mirror, the beam-scaled per-source sum and through the solver
layer. Limits are max |err| / max |ref| per cluster."""
import numpy as np
import pytest
import torch

import shapelet_sky as S
from sagecal_amd.ops import reference as R
from sagecal_amd.ops import hip_host

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FREQS = (S.FREQ0, 1.02 * S.FREQ0)


@pytest.fixture(scope='module')
def sky():
    """Standard sky, rows on host and device, fp64 references per freq."""
    pack, gis = S.make_pack()
    u, v, w, bb, Nbase = S.uvw_rows()
    refs = {f: R.predict_coh(pack, u, v, w, f, S.FREQ0, S.FDELTA, S.TDELTA,
                             S.DEC0) for f in FREQS}
    uvw_d = tuple(t.to(DEV) for t in (u, v, w))
    return dict(pack=pack, gis=gis, uvw=(u, v, w), uvw_d=uvw_d, bb=bb,
                Nbase=Nbase, refs=refs)


def _gpu_predict(sky, freq, **kw):
    return hip_host.predict_coh(sky['pack'], *sky['uvw_d'], freq, S.FREQ0,
                                S.FDELTA, S.TDELTA, S.DEC0, **kw)


@pytest.mark.parametrize('freq', FREQS)
def test_kernel_matches_reference(sky, freq):
    got = _gpu_predict(sky, freq)
    err = S.cluster_err(got, sky['refs'][freq])
    print('kernel vs fp64 reference, per cluster:', err)
    assert max(err) < 1e-5, err


def test_no_host_loop(sky, monkeypatch):
    """The GPU predict never reaches the per-source torch envelope."""
    from sagecal_amd import shapelet

    def boom(*a, **k):
        raise AssertionError('shapelet_contrib called on the GPU path')
    monkeypatch.setattr(shapelet, 'shapelet_contrib', boom)
    got = _gpu_predict(sky, S.FREQ0)
    err = S.cluster_err(got, sky['refs'][S.FREQ0])
    assert max(err) < 1e-5, err


@pytest.mark.parametrize('freq', FREQS)
def test_kernel_matches_mirror(sky, freq, monkeypatch):
    monkeypatch.delenv('SAGECAL_SHAPELET_HOST', raising=False)
    kern = _gpu_predict(sky, freq)
    monkeypatch.setenv('SAGECAL_SHAPELET_HOST', '1')
    mirr = _gpu_predict(sky, freq)
    assert not torch.equal(kern, mirr)      # two different code paths ran
    err = S.cluster_err(kern, mirr)
    print('kernel vs mirror, per cluster:', err)
    assert max(err) < 1e-5, err


def test_beam_scales_every_source(sky):
    """Random positive beam [T, K, N]: every source type, shapelets
    included, is scaled by beam[t,g,p] beam[t,g,q]."""
    pack, bb, Nbase = sky['pack'], sky['bb'], sky['Nbase']
    rng = np.random.default_rng(5)
    beam = torch.tensor(rng.uniform(0.2, 1.0, (3, pack.K, 10)),
                        dtype=torch.float32)
    ref = S.beamed_reference(pack, range(pack.K), beam, bb, Nbase,
                             *sky['uvw'], S.FREQ0)
    got = _gpu_predict(sky, S.FREQ0, beam=beam.to(DEV),
                       pairs=bb[:Nbase].to(device=DEV, dtype=torch.int32),
                       Nbase=Nbase)
    err = S.cluster_err(got, ref)
    print('beamed kernel vs per-source sum, per cluster:', err)
    assert max(err) < 1e-5, err


def test_predict_withbeam_gpu_matches_cpu(sky):
    """beams.predict_coh_withbeam(mode=1) gives the same answer on the GPU
    (fused kernels) and on the CPU for a sky with shapelets."""
    from sagecal_amd import beams
    pack, bb, Nbase = sky['pack'], sky['bb'], sky['Nbase']
    N, T = 10, 3
    tmjd = np.array([57000.0, 57000.0001, 57000.0002])
    rng2 = np.random.default_rng(7)
    elems = [rng2.uniform(-30, 30, (16, 3)) for _ in range(N)]
    cfg = beams.ArrayConfig(elems, 0.1, 0.92, 0.0, S.DEC0)
    tail = (S.FREQ0, S.FREQ0, S.FDELTA, S.TDELTA, S.DEC0, cfg, tmjd)
    cpu = beams.predict_coh_withbeam(pack, *sky['uvw'], *tail, bb, Nbase, T,
                                     mode=1)
    gpu = beams.predict_coh_withbeam(pack, *sky['uvw_d'], *tail, bb.to(DEV),
                                     Nbase, T, mode=1)
    err = float((gpu.cpu().to(cpu.dtype) - cpu).abs().max()
                / cpu.abs().max())
    assert err < 2e-4, err
    perc = S.cluster_err(gpu, cpu)
    print('withbeam gpu vs cpu, per cluster:', perc)
    assert max(perc) < 2e-4, perc


def test_precalc_coherencies_two_channels(sky):
    """Through the solver layer: a 2-channel tile predicts per channel."""
    from sagecal_amd.solvers import sage

    class Tile:
        pass
    tiles = {}
    for name, uvw in (('cpu', sky['uvw']), ('gpu', sky['uvw_d'])):
        t = Tile()
        t.u, t.v, t.w = uvw
        t.freqs = np.array([S.FREQ0 - 1e6, S.FREQ0 + 1e6])
        t.freq0, t.fdelta, t.tdelta, t.dec0 = S.FREQ0, 4e6, S.TDELTA, S.DEC0
        tiles[name] = t
    ref = sage.precalc_coherencies(sky['pack'], tiles['cpu'])
    got = sage.precalc_coherencies(sky['pack'], tiles['gpu'])
    assert got.is_cuda
    err = S.cluster_err(got, ref)
    print('precalc_coherencies gpu vs cpu, per cluster:', err)
    assert max(err) < 1e-5, err


def test_no_shapelets_is_the_plain_kernel(sky):
    pack, _ = S.make_pack(spec=())
    gp = hip_host.gpu_pack(pack, torch.device(DEV))
    assert gp.sh is None
    u, v, w = sky['uvw_d']
    got = hip_host.predict_coh(pack, u, v, w, S.FREQ0, S.FREQ0, S.FDELTA,
                               S.TDELTA, S.DEC0)
    sI, sQ, sU, sV = gp.fluxes_at(S.FREQ0, S.FREQ0)
    direct = hip_host._ext().predict_coh(
        u, v, w, gp.ll, gp.mm, gp.nn1, sI, sQ, sU, sV, gp.eX, gp.eY, gp.eP,
        gp.cxi, gp.sxi, gp.cphi, gp.sphi, gp.r1_for(S.DEC0), gp.stype,
        gp.cluster_off, S.FREQ0, S.FDELTA * 0.5, S.TDELTA)
    assert torch.equal(got, direct.view(pack.M, -1, 2, 2))


def test_cluster_of_one_shapelet(sky):
    """Cluster 0 holds nothing but a shapelet: the main kernel writes
    zeros there and the shapelet kernel supplies the whole result."""
    pack, gis = S.make_pack(
        spec=((0, 0, 5, 1.5e-3, True, 0.8, 1.3, 0.4),), M=2, nsrc=1)
    assert gis == [0] and int(pack.cluster_off[1]) == 1
    ref = R.predict_coh(pack, *sky['uvw'], S.FREQ0, S.FREQ0, S.FDELTA,
                        S.TDELTA, S.DEC0)
    got = hip_host.predict_coh(pack, *sky['uvw_d'], S.FREQ0, S.FREQ0,
                               S.FDELTA, S.TDELTA, S.DEC0)
    assert float(got[0].abs().max()) > 0.0
    err = S.cluster_err(got, ref)
    assert max(err) < 1e-5, err
