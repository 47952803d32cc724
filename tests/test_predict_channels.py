"""ops.predict_coh_channels and ops.residuals_multifreq on the CPU, where
they are the per-channel loop over the fp64 reference, and
sage.calculate_residuals_multifreq there, which does not use them."""
import pytest
import torch

import channels_case as C
import shapelet_sky as S
from sagecal_amd import sky
from sagecal_amd.ops import dispatch as ops
from sagecal_amd.ops import reference as R
from sagecal_amd.solvers import sage

N = 10
FREQS = C.channels(5, 5)


@pytest.fixture(scope='module')
def case():
    srcs, clist = sky.make_synthetic_sky(M=4, nsrc_per_cluster=3, seed=21)
    pack = R.SourcePack(sky.build_clusters(srcs, clist, 0.0, S.DEC0,
                                           S.FREQ0))
    C.set_chunks_and_ids(pack)
    u, v, w, bb, Nbase = S.uvw_rows()
    tile = C.make_tile((u, v, w), Nbase, FREQS)
    state = C.random_state(pack, N)
    assert state.Mt == sum(C.NCHUNK)
    per_channel = [R.predict_coh(pack, u, v, w, f, S.FREQ0, S.FDELTA,
                                 S.TDELTA, S.DEC0) for f in FREQS]
    return dict(pack=pack, tile=tile, bb=bb, Nbase=Nbase, state=state,
                per_channel=per_channel)


def predict(case, freqs, **kw):
    t = case['tile']
    return ops.predict_coh_channels(case['pack'], t.u, t.v, t.w, freqs,
                                    S.FREQ0, S.FDELTA, S.TDELTA, S.DEC0,
                                    **kw)


def test_channels_are_the_stack_of_single_predicts(case):
    got = predict(case, FREQS)
    assert got.shape == (len(FREQS), 4, 135, 2, 2)
    assert torch.equal(got, torch.stack(case['per_channel']))


def test_mean_is_the_channel_mean(case):
    got = predict(case, FREQS, reduce='mean')
    want = torch.stack(case['per_channel']).mean(dim=0)
    assert got.shape == want.shape
    assert float((got - want).abs().max() / want.abs().max()) < 1e-14


def test_empty_and_bad_arguments(case):
    assert predict(case, []).shape == (0, 4, 135, 2, 2)
    with pytest.raises(ValueError):
        predict(case, [], reduce='mean')
    with pytest.raises(ValueError):
        predict(case, FREQS, reduce='sum')


def chunk_table(state, T):
    """[M, T] global chunk ids, written out: chunks split the T slots in
    runs of ceil(T / nchunk), the remainder to the last."""
    tab = torch.zeros(state.M, T, dtype=torch.int32)
    for ci, nc in enumerate(state.nchunks):
        tpc = -(-T // nc)
        for t in range(T):
            tab[ci, t] = state.chunk_off[ci] + min(t // tpc, nc - 1)
    return tab


def test_chunk_table_of_the_hybrid_state(case):
    tab = chunk_table(case['state'], 3)
    assert tab.tolist() == [[0, 0, 0], [1, 1, 2], [3, 4, 5], [6, 6, 6]]
    assert torch.equal(sage._chunk_table(case['state'], 3, 45, 'cpu'), tab)


def test_residuals_are_data_minus_total_model(case):
    pack, tile, bb, state = (case[k] for k in ('pack', 'tile', 'bb', 'state'))
    T, Nbase = tile.tilesz, tile.Nbase
    subtract = [c >= 0 for c in pack.cluster_ids]
    assert subtract == [True, False, True, True]
    got = ops.residuals_multifreq(
        pack, tile.xo, tile.u, tile.v, tile.w, FREQS, S.FREQ0, S.FDELTA,
        S.TDELTA, S.DEC0, state.J, chunk_table(state, T), bb[:Nbase],
        subtract=subtract)
    assert got.shape == tile.xo.shape
    for fi, coh in enumerate(case['per_channel']):
        want = tile.xo[fi] - sage.total_model(state, coh, bb, T, Nbase,
                                              skip={1})
        assert torch.equal(got[fi], want), fi
    # the mask matters: cluster 1 left in changes the answer
    full = ops.residuals_multifreq(
        pack, tile.xo, tile.u, tile.v, tile.w, FREQS, S.FREQ0, S.FDELTA,
        S.TDELTA, S.DEC0, state.J, chunk_table(state, T), bb[:Nbase])
    assert float((full - got).abs().max()) > 1e-3 * float(got.abs().max())


def test_negative_pair_keeps_the_data(case):
    pack, tile, bb, state = (case[k] for k in ('pack', 'tile', 'bb', 'state'))
    T, Nbase = tile.tilesz, tile.Nbase
    args = (pack, tile.xo, tile.u, tile.v, tile.w, FREQS, S.FREQ0, S.FDELTA,
            S.TDELTA, S.DEC0, state.J, chunk_table(state, T))
    ref = ops.residuals_multifreq(*args, bb[:Nbase])
    pairs = bb[:Nbase].clone()
    pairs[7, 1] = -1
    got = ops.residuals_multifreq(*args, pairs)
    hit = torch.arange(T) * Nbase + 7
    assert torch.equal(got[:, hit], tile.xo[:, hit])
    keep = torch.ones(T * Nbase, dtype=torch.bool)
    keep[hit] = False
    assert torch.equal(got[:, keep], ref[:, keep])


def test_sage_residuals_on_the_cpu_take_the_loop(case, monkeypatch):
    """calculate_residuals_multifreq on CPU tensors never calls the new
    entry point, and gives data minus total_model per channel."""
    pack, tile, bb, state = (case[k] for k in ('pack', 'tile', 'bb', 'state'))

    def never(*a, **k):
        raise AssertionError("the CPU path must not call this")
    monkeypatch.setattr(ops, 'residuals_multifreq', never, raising=False)
    monkeypatch.setattr(ops, 'predict_coh_channels', never, raising=False)
    got = sage.calculate_residuals_multifreq(state, pack, tile, bb)
    for fi, coh in enumerate(case['per_channel']):
        want = tile.xo[fi] - sage.total_model(state, coh, bb, tile.tilesz,
                                              tile.Nbase, skip={1})
        assert torch.equal(got[fi], want), fi
    mean = sage.precalc_coherencies(pack, tile)
    want = torch.stack(case['per_channel']).mean(dim=0)
    assert float((mean - want).abs().max() / want.abs().max()) < 1e-14
