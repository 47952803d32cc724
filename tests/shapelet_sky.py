"""The sky and uvw rows shared by the shapelet-kernel tests
(test_shapelet_table.py, test_gpu_shapelet_kernel.py).

Standard sky: 3 clusters x 3 sources. Cluster 0 holds two shapelet sources
(n0=1; n0=5 with use_proj on, eX=0.8, eY=1.3, eP=0.4), cluster 1 none,
cluster 2's LAST source is a shapelet with n0=12, beta=3e-3, use_proj off.
The shapelet sources carry non-zero Q, U, V. Rows: the 135 baselines x
timeslots of SyntheticMS(N=10, tilesz=3) — one full 128-thread block plus a
7-row tail.
"""
import numpy as np
import torch

FREQ0 = 150e6
DEC0 = np.pi / 4
FDELTA = 30e3
TDELTA = 5.0

# (cluster, source in cluster, n0, beta, use_proj, eX, eY, eP)
STANDARD = ((0, 0, 1, 1.0e-3, False, 1.0, 1.0, 0.0),
            (0, 1, 5, 1.5e-3, True, 0.8, 1.3, 0.4),
            (2, 2, 12, 3.0e-3, False, 1.0, 1.0, 0.0))


def make_pack(spec=STANDARD, M=3, nsrc=3, seed=9):
    """SourcePack with the sources of `spec` turned into shapelets.
    Returns (pack, sorted global indices of the shapelet sources)."""
    from sagecal_amd import sky
    from sagecal_amd.ops.reference import SourcePack
    srcs, clist = sky.make_synthetic_sky(M=M, nsrc_per_cluster=nsrc,
                                         seed=seed)
    rng = np.random.default_rng(seed + 100)
    for ci, si, n0, beta, _proj, _eX, _eY, _eP in spec:
        s = srcs[clist[ci][2][si]]
        s.stype = 4
        s.eX = s.eY = 1.0
        s.sQ, s.sU, s.sV = 0.3 * s.sI, -0.2 * s.sI, 0.1 * s.sI
        s.sh_n0 = n0
        s.sh_beta = beta
        k = np.arange(n0)
        decay = 1.0 / (1.0 + k[None, :] + k[:, None])
        s.sh_coeff = (rng.uniform(-1.0, 1.0, (n0, n0)) * decay).reshape(-1)
        s.sh_coeff[0] = 1.0
    clusters = sky.build_clusters(srcs, clist, 0.0, DEC0, FREQ0)
    pack = SourcePack(clusters)
    gis = []
    # set on the pack BEFORE any GPU call: gpu_pack caches per pack object
    for ci, si, _n0, _beta, proj, eX, eY, eP in spec:
        gi = int(pack.cluster_off[ci]) + si
        pack.use_proj[gi] = int(proj)
        pack.eX[gi], pack.eY[gi], pack.eP[gi] = eX, eY, eP
        gis.append(gi)
    assert sorted(pack.shapelets) == sorted(gis)
    return pack, sorted(gis)


def zero_fluxes(pack, gis):
    """Zero every flux of sources `gis` in place (for reference
    differences); returns the pack."""
    for k in ('sI', 'sQ', 'sU', 'sV', 'sI0', 'sQ0', 'sU0', 'sV0'):
        getattr(pack, k)[gis] = 0.0
    return pack


def uvw_rows():
    """(u, v, w) [135] float64 seconds, Nbase=45, T=3, and the station
    pair table [135, 2]."""
    from sagecal_amd import msdata
    ms = msdata.SyntheticMS(N=10, tilesz=3, Ntime=3, Nchan=1, pack=None,
                            seed=13)
    tile = ms.load_tile(0)
    assert tile.u.shape[0] == 135
    return tile.u, tile.v, tile.w, ms.bb_tensor(device='cpu'), tile.Nbase


def cluster_err(got, ref):
    """max |got - ref| / max |ref| per cluster, as a list of floats.
    got, ref: [M, B, 2, 2]."""
    got = got.detach().cpu().to(torch.complex128)
    ref = ref.detach().cpu().to(torch.complex128)
    M = ref.shape[0]
    num = (got - ref).abs().reshape(M, -1).max(dim=1).values
    den = ref.abs().reshape(M, -1).max(dim=1).values
    return [float(n / d) for n, d in zip(num, den)]


def beamed_reference(pack, gis, beam, bb, Nbase, u, v, w, freq):
    """Sum over sources `gis` of beam[t,g,p] beam[t,g,q] times the fp64
    single-source coherency, scattered to the sources' clusters:
    [M, B, 2, 2] complex128. beam: [T, K, N]."""
    from sagecal_amd import beams
    B = u.shape[0]
    t = torch.arange(B) // Nbase
    p, q = bb[:, 0].long(), bb[:, 1].long()
    co = pack.cluster_off.tolist()
    out = torch.zeros(pack.M, B, 2, 2, dtype=torch.complex128)
    bd = beam.to(torch.float64)
    for g in gis:
        ci = max(c for c in range(pack.M) if co[c] <= g)
        sub = beams._single_source_coh(pack, g, u, v, w, freq, FREQ0,
                                       FDELTA, TDELTA, DEC0)
        out[ci] += (bd[t, g, p] * bd[t, g, q])[:, None, None] * sub
    return out
