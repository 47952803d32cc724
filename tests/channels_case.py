"""Shared pieces of the all-channels predict tests
(test_predict_channels.py, test_gpu_predict_channels.py): the channel
grid, a tile of the 135 rows of shapelet_sky.uvw_rows() with drawn data,
and a calibration state with random solutions."""
from types import SimpleNamespace

import torch

import shapelet_sky as S

SPACING = 200e3
NCHUNK = (1, 2, 3, 1)


def channels(F, Fmax):
    """F adjacent channels of the grid FREQ0 + SPACING * (k - Fmax // 2),
    k < Fmax, chosen around its middle: every set holds FREQ0 itself."""
    c = Fmax // 2
    lo = c - F // 2
    assert 0 <= lo and lo + F <= Fmax
    return [S.FREQ0 + SPACING * (k - c) for k in range(lo, lo + F)]


def make_tile(uvw, Nbase, freqs, seed=5, dtype=torch.complex128):
    """Tile-like object on the CPU. xo is drawn in complex64 and widened,
    so a complex64 copy on a device holds the same values."""
    u, v, w = uvw
    B = u.shape[0]
    g = torch.Generator().manual_seed(seed)
    xo = torch.complex(torch.randn(len(freqs), B, 2, 2, generator=g),
                       torch.randn(len(freqs), B, 2, 2, generator=g))
    xo = (20.0 * xo).to(torch.complex64)
    return SimpleNamespace(
        u=u, v=v, w=w, x=xo[0].to(dtype), xo=xo.to(dtype),
        freqs=list(freqs), freq0=S.FREQ0, fdelta=S.FDELTA * len(freqs),
        tdelta=S.TDELTA, dec0=S.DEC0, tilesz=B // Nbase, Nbase=Nbase)


def to_device(tile, dev):
    """complex64 copy of a make_tile() tile on `dev`."""
    t = SimpleNamespace(**vars(tile))
    for k in ('u', 'v', 'w'):
        setattr(t, k, getattr(tile, k).to(dev))
    t.x = tile.x.to(device=dev, dtype=torch.complex64)
    t.xo = tile.xo.to(device=dev, dtype=torch.complex64)
    return t


def random_state(pack, N, seed=3, device='cpu', dtype=torch.complex128):
    """CalState with J = I + 0.3 (randn + i randn), drawn on the CPU in
    fp64 whatever the device, so every copy holds the same solutions."""
    from sagecal_amd.solvers import sage
    state = sage.CalState(pack, N, device=device, dtype=dtype)
    g = torch.Generator().manual_seed(seed)
    shape = (state.Mt, N, 2, 2)
    d = torch.complex(torch.randn(shape, generator=g, dtype=torch.float64),
                      torch.randn(shape, generator=g, dtype=torch.float64))
    state.J = (torch.eye(2, dtype=torch.complex128) + 0.3 * d).to(
        device=device, dtype=dtype)
    return state


def set_chunks_and_ids(pack, nchunk=NCHUNK, negative=1):
    """Hybrid chunk counts on the pack, and cluster `negative` given a
    negative id (solved, not subtracted)."""
    assert len(nchunk) == pack.M
    pack.nchunk = torch.tensor(nchunk, dtype=torch.long)
    ids = list(range(pack.M))
    if negative is not None:
        ids[negative] = -7
    pack.cluster_ids = ids
    return pack
