"""k_predict_coh at the edges of its 64-source LDS tile: one pack with
clusters of 1, 64, 65 and 130 sources (one tile, an exactly full tile,
full plus one, two full plus two), extended sources in second-tile slots,
negative and polarised fluxes, against the fp64 reference on the same
rows. Limit: per-cluster max|err| / max|ref| < 1e-5, the one
test_gpu_shapelet_kernel.py holds this kernel to."""
import numpy as np
import pytest
import torch

import shapelet_sky as S
from sagecal_amd.ops import reference as R
from sagecal_amd.ops import hip_host

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
LIMIT = 1e-5
SIZES = (1, 64, 65, 130)
FREQS = (S.FREQ0, 1.02 * S.FREQ0)
ROWSETS = ('all135', 'first128', 'first1', 'zero', 'long')


def make_edge_pack():
    """Clusters of SIZES sources. In the 65- and 130-source clusters
    every fourth source is extended: gaussian, disk, ring in turn (sizes
    of test_gpu.py's `problem` fixture; gaussians elliptical with
    non-zero eP, every other one projected). Source i of a cluster has
    negative I when i % 10 == 3 and carries Q, U, V when i % 3 == 1."""
    from sagecal_amd import sky
    srcs, clist = sky.make_synthetic_sky(M=len(SIZES),
                                         nsrc_per_cluster=max(SIZES), seed=17)
    clist = [(cid, nch, names[:n])
             for (cid, nch, names), n in zip(clist, SIZES)]
    gauss = []                      # (cluster, position) of the gaussians
    for ci, (_cid, _nch, names) in enumerate(clist):
        for i, name in enumerate(names):
            s = srcs[name]
            if i % 10 == 3:
                s.sI = -s.sI
            if i % 3 == 1:
                s.sQ, s.sU, s.sV = 0.3 * s.sI, -0.2 * s.sI, 0.1 * s.sI
            if len(names) < 65 or i % 4:
                continue
            s.stype = (1, 2, 3)[(i // 4) % 3]
            if s.stype == 1:
                s.eX, s.eY, s.eP = 0.001, 0.0006, 0.4 + 0.01 * i
                gauss.append((ci, i))
            else:
                s.eX = s.eY = 0.0007 if s.stype == 2 else 0.0005
    clusters = sky.build_clusters(srcs, clist, 0.0, S.DEC0, S.FREQ0)
    pack = R.SourcePack(clusters)
    # set on the pack BEFORE any GPU call: gpu_pack caches per pack object
    for k, (ci, i) in enumerate(gauss):
        pack.use_proj[int(pack.cluster_off[ci]) + i] = k % 2
    return pack


@pytest.fixture(scope='module')
def edge():
    """The pack, the row sets, and the fp64 reference of every
    (row set, frequency), computed once."""
    pack = make_edge_pack()
    co = pack.cluster_off.tolist()
    assert [b - a for a, b in zip(co, co[1:])] == list(SIZES)
    st = pack.stype
    # a second-tile slot of each extended type, and both gaussian modes
    assert int(st[co[2] + 64]) != 0
    assert {int(t) for t in st[co[3] + 64:co[4]]} == {0, 1, 2, 3}
    g = st == 1
    assert int(pack.use_proj[g].sum()) not in (0, int(g.sum()))
    assert float(pack.eP[g].abs().min()) > 0.0
    assert int((pack.sI < 0).sum()) == 27 and int((pack.sV != 0).sum()) == 86

    u, v, w, _bb, _Nbase = S.uvw_rows()
    uvw = torch.stack([u, v, w])                       # [3, 135]
    k = 3e-3 / float(uvw.abs().max())
    rowsets = {'all135': uvw, 'first128': uvw[:, :128].contiguous(),
               'first1': uvw[:, :1].contiguous(),
               'zero': torch.zeros(3, 1, dtype=torch.float64),
               'long': uvw * k}
    assert abs(float(rowsets['long'].abs().max()) - 3e-3) < 1e-12
    refs = {(n, f): R.predict_coh(pack, *rs, f, S.FREQ0, S.FDELTA, S.TDELTA,
                                  S.DEC0)
            for n, rs in rowsets.items() for f in FREQS}
    return dict(pack=pack, rowsets=rowsets, refs=refs)


def gpu_predict(pack, uvw, freq, fdelta=S.FDELTA):
    u, v, w = (t.to(DEV) for t in uvw)
    return hip_host.predict_coh(pack, u, v, w, freq, S.FREQ0, fdelta,
                                S.TDELTA, S.DEC0)


@pytest.mark.parametrize('freq', FREQS)
@pytest.mark.parametrize('rows', ROWSETS)
def test_source_tile_edges(edge, rows, freq):
    got = gpu_predict(edge['pack'], edge['rowsets'][rows], freq)
    ref = edge['refs'][rows, freq]
    assert got.shape == ref.shape
    err = S.cluster_err(got, ref)
    print(f"{rows} @ {freq / 1e6:.0f} MHz, clusters of {SIZES}: "
          + ' '.join(f'{e:.2e}' for e in err))
    assert max(err) < LIMIT, err


@pytest.mark.parametrize('freq', FREQS)
def test_zero_baseline_is_the_flux_sum(edge, freq):
    """u = v = w = 0: no phase, no smearing (the G = 0 and prod = 0
    branches), gaussian and ring envelopes 1 and the disk's j1(0) = 0, so
    each cluster's coherency is the plain sum of its non-disk fluxes."""
    pack = edge['pack']
    got = gpu_predict(pack, edge['rowsets']['zero'], freq)
    got = got.cpu().to(torch.complex128)[:, 0]              # [M, 2, 2]
    co = pack.cluster_off.tolist()
    for ci in range(pack.M):
        sel = slice(co[ci], co[ci + 1])
        keep = (pack.stype[sel] != 2).to(torch.float64)
        I, Q, U, V = (f * keep for f in
                      R._source_flux_at(pack, sel, float(freq), S.FREQ0))
        want = torch.stack([(I + Q).sum() + 0j, (U + 1j * V).sum(),
                            (U - 1j * V).sum(), (I - Q).sum() + 0j])
        err = float((got[ci].reshape(4) - want).abs().max()
                    / want.abs().max())
        print(f"zero row @ {freq / 1e6:.0f} MHz cluster {ci}: {err:.2e}")
        assert err < LIMIT, (ci, err)
