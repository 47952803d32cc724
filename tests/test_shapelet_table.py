"""ShapeletTable contract and the torch mirror of k_shapelet_coh, on the
CPU: the table layout the kernel reads, and the mirror's arithmetic against
the fp64 reference predict."""
import math

import numpy as np
import pytest
import torch

import shapelet_sky as S
from sagecal_amd.ops import reference as R
from sagecal_amd.ops import hip_host


@pytest.fixture(scope='module')
def sky():
    pack, gis = S.make_pack()
    u, v, w, bb, Nbase = S.uvw_rows()
    return pack, gis, u, v, w, bb, Nbase


def test_table_contract(sky):
    pack, gis, *_ = sky
    tab = hip_host.ShapeletTable(pack, 'cpu')
    assert gis == [0, 1, 8]
    assert tab.src.dtype == torch.int32 and tab.src.tolist() == gis
    assert tab.cluster.dtype == torch.int32
    assert tab.cluster.tolist() == [0, 0, 2]
    assert tab.n0.dtype == torch.int32 and tab.n0.tolist() == [1, 5, 12]
    assert tab.off.dtype == torch.int32
    assert tab.off.tolist() == [0, 1, 26, 170]
    assert tab.psign.tolist() == [1.0, -1.0, 1.0]
    for k in ('beta', 'coef', 'cxi', 'sxi', 'cphi', 'sphi', 'psign', 'a',
              'b', 'ceP', 'seP', 'rec'):
        assert getattr(tab, k).dtype == torch.float32, k
    for k in ('ll', 'mm', 'nn1'):
        assert getattr(tab, k).dtype == torch.float64, k
        assert torch.equal(getattr(tab, k), getattr(pack, k)[gis])
    # identity rotation baked where use_proj is off, pack values where on
    for s in (0, 2):
        assert (tab.cxi[s], tab.sxi[s], tab.cphi[s], tab.sphi[s]) == \
            (1.0, 0.0, 1.0, 0.0)
    for k in ('cxi', 'sxi', 'cphi', 'sphi'):
        assert float(getattr(tab, k)[1]) == \
            float(getattr(pack, k)[gis[1]].to(torch.float32))
    assert float(pack.sxi[gis[1]]) != 0.0
    f32 = lambda x: float(np.float32(x))
    assert float(tab.a[1]) == f32(1 / 0.8) and float(tab.b[1]) == f32(1 / 1.3)
    assert float(tab.ceP[1]) == f32(math.cos(0.4))
    assert float(tab.seP[1]) == f32(math.sin(0.4))
    # coef == modes * sgn(n1+n2) * 2 pi / (eX eY), element by element
    assert tab.coef.shape == (170,)
    for s, gi in enumerate(gis):
        n0, beta, modes = pack.shapelets[gi]
        assert float(tab.beta[s]) == f32(beta)
        eX, eY = float(pack.eX[gi]), float(pack.eY[gi])
        for n2 in range(n0):
            for n1 in range(n0):
                sgn = 1.0 if (n1 + n2) % 4 in (0, 1) else -1.0
                want = modes[n2 * n0 + n1] * sgn * 2 * math.pi / (eX * eY)
                got = float(tab.coef[int(tab.off[s]) + n2 * n0 + n1])
                assert got == pytest.approx(want, rel=2e-7, abs=0), \
                    (s, n1, n2)
    # recurrence constants
    assert tab.rec.shape == (2, 12)
    n = np.arange(1, 12)
    np.testing.assert_allclose(tab.rec[0, 1:].numpy(), np.sqrt(2.0 / n),
                               rtol=1e-7)
    np.testing.assert_allclose(tab.rec[1, 1:].numpy(),
                               np.sqrt((n - 1.0) / n), rtol=1e-7)


def test_gpupack_exposes_table(sky):
    """gp.sh is the table (None without shapelets), the main-kernel fluxes
    of shapelet sources are zero, and the gathered [4, S] float32 fluxes
    follow the spectral index like the fp64 reference."""
    pack, gis, *_ = sky
    gp = hip_host.GPUPack(pack, 'cpu')
    assert isinstance(gp.sh, hip_host.ShapeletTable)
    for freq in (S.FREQ0, 1.02 * S.FREQ0):
        main = gp.fluxes_at(freq, S.FREQ0)
        assert all(float(f[gis].abs().max()) == 0.0 for f in main)
        flux = gp.shapelet_fluxes_at(freq, S.FREQ0)
        assert flux.shape == (4, 3) and flux.dtype == torch.float32
        want = torch.stack(R._source_flux_at(pack, gis, freq, S.FREQ0))
        assert float(want.abs().min()) > 0.0
        # fp32 log/exp of fluxes within e^+-3: a few ulp of |log flux| <= 3
        assert float(((flux.double() - want) / want).abs().max()) < 2e-6
    plain, _ = S.make_pack(spec=())
    assert hip_host.GPUPack(plain, 'cpu').sh is None


@pytest.mark.parametrize('fscale', [1.0, 1.02])
def test_mirror_matches_reference_fp64(sky, fscale):
    """fp64 mirror (table built unrounded) vs the reference's shapelet
    part: predict(pack) - predict(pack with shapelet fluxes zeroed). Both
    are fp64 evaluations of the same closed form, so 1e-9 of the
    per-cluster maximum only admits rounding."""
    pack, gis, u, v, w, *_ = sky
    freq = fscale * S.FREQ0
    args = (u, v, w, freq, S.FREQ0, S.FDELTA, S.TDELTA, S.DEC0)
    full = R.predict_coh(pack, *args)
    rest = R.predict_coh(S.zero_fluxes(S.make_pack()[0], gis), *args)
    ref = full - rest
    tab = hip_host.ShapeletTable(pack, 'cpu', dtype=torch.float64)
    flux = torch.stack(R._source_flux_at(pack, gis, freq, S.FREQ0))
    r1 = torch.sqrt(pack.ll ** 2 + (math.sin(S.DEC0) * pack.mm) ** 2)[gis]
    got = hip_host.shapelet_coh_torch(tab, flux, r1, u, v, w, freq,
                                      S.FDELTA, S.TDELTA)
    assert got.dtype == torch.complex128 and got.shape == ref.shape
    assert float(got[1].abs().max()) == 0.0      # cluster 1: no shapelets
    for ci in (0, 2):
        # the shapelet part is no rounding residue of the difference
        assert float(ref[ci].abs().max()) > 0.01 * float(full[ci].abs().max())
        err = float((got[ci] - ref[ci]).abs().max() / ref[ci].abs().max())
        print('fp64 mirror err cluster', ci, err)
        assert err < 1e-9, (ci, err)


def test_mirror_with_beam(sky):
    """Mirror with a random beam [T, K, N] vs the per-source sum of
    beam[t,g,p] beam[t,g,q] x single-source coherency over the shapelet
    sources only."""
    pack, gis, u, v, w, bb, Nbase = sky
    rng = np.random.default_rng(5)
    beam = torch.tensor(rng.uniform(0.2, 1.0, (3, pack.K, 10)))
    ref = S.beamed_reference(pack, gis, beam, bb, Nbase, u, v, w, S.FREQ0)
    tab = hip_host.ShapeletTable(pack, 'cpu', dtype=torch.float64)
    flux = torch.stack(R._source_flux_at(pack, gis, S.FREQ0, S.FREQ0))
    r1 = torch.sqrt(pack.ll ** 2 + (math.sin(S.DEC0) * pack.mm) ** 2)[gis]
    got = hip_host.shapelet_coh_torch(
        tab, flux, r1, u, v, w, S.FREQ0, S.FDELTA, S.TDELTA, beam=beam,
        pairs=bb[:Nbase].to(torch.int32), Nbase=Nbase)
    for ci in (0, 2):
        err = float((got[ci] - ref[ci]).abs().max() / ref[ci].abs().max())
        print('beamed mirror err cluster', ci, err)
        assert err < 1e-9, (ci, err)
    assert float(got[1].abs().max()) == 0.0
