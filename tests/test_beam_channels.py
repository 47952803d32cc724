"""The beam arguments of ops.predict_coh_channels, ops.residuals_multifreq
and sage.calculate_residuals_multifreq on the CPU, where the beamed case
stays with the per-channel loop over beams.predict_coh_withbeam."""
import numpy as np
import pytest
import torch

import channels_case as C
import shapelet_sky as S
from sagecal_amd import beams, sky
from sagecal_amd.ops import dispatch as ops
from sagecal_amd.ops import reference as R
from sagecal_amd.solvers import sage

N, T = 10, 3
FREQS = C.channels(3, 3)


@pytest.fixture(scope='module')
def case():
    srcs, clist = sky.make_synthetic_sky(M=4, nsrc_per_cluster=2, seed=21)
    pack = R.SourcePack(sky.build_clusters(srcs, clist, 0.0, S.DEC0,
                                           S.FREQ0))
    C.set_chunks_and_ids(pack)
    u, v, w, bb, Nbase = S.uvw_rows()
    tile = C.make_tile((u, v, w), Nbase, FREQS)
    state = C.random_state(pack, N)
    K, F = int(pack.cluster_off[-1]), len(FREQS)
    rng = np.random.default_rng(5)
    gains = torch.tensor(rng.uniform(0.2, 1.0, (F, T, K, N)))
    ej = torch.tensor(rng.uniform(-1, 1, (F, T, K, 2, 2))
                      + 1j * rng.uniform(-1, 1, (F, T, K, 2, 2)))
    return dict(pack=pack, tile=tile, bb=bb, Nbase=Nbase, state=state,
                gains=gains, ej=ej)


def withbeam(case, fi, mode):
    """beams.predict_coh_withbeam of channel fi with the case's buffers."""
    t = case['tile']
    return beams.predict_coh_withbeam(
        case['pack'], t.u, t.v, t.w, FREQS[fi], S.FREQ0, S.FDELTA, S.TDELTA,
        S.DEC0, None, None, case['bb'], case['Nbase'], T, mode=mode, geom=(),
        gains=case['gains'][fi] if mode in (1, 2) else None,
        ejones=case['ej'][fi] if mode in (2, 3) else None)


def chunk_table(state):
    return sage._chunk_table(state, T, 45, 'cpu')


def test_new_arguments_default_to_the_unbeamed_calls(case):
    pack, t, state = case['pack'], case['tile'], case['state']
    args = (pack, t.u, t.v, t.w, FREQS, S.FREQ0, S.FDELTA, S.TDELTA, S.DEC0)
    plain = ops.predict_coh_channels(*args)
    assert torch.equal(plain, ops.predict_coh_channels(
        *args, beam=None, ejones=None, pairs=None, Nbase=0))
    assert torch.equal(
        ops.predict_coh_channels(*args, reduce='mean'),
        ops.predict_coh_channels(*args, reduce='mean', beam=None,
                                 ejones=None))
    rargs = (pack, t.xo, t.u, t.v, t.w, FREQS, S.FREQ0, S.FDELTA, S.TDELTA,
             S.DEC0, state.J, chunk_table(state), case['bb'][:45])
    assert torch.equal(ops.residuals_multifreq(*rargs),
                       ops.residuals_multifreq(*rargs, beam=None,
                                               ejones=None))


@pytest.mark.parametrize('mode', [1, 2, 3])
def test_beamed_channels_are_the_withbeam_loop(case, mode):
    pack, t = case['pack'], case['tile']
    kw = dict(pairs=case['bb'][:45], Nbase=45)
    if mode in (1, 2):
        kw['beam'] = case['gains']
    if mode in (2, 3):
        kw['ejones'] = case['ej']
    got = ops.predict_coh_channels(pack, t.u, t.v, t.w, FREQS, S.FREQ0,
                                   S.FDELTA, S.TDELTA, S.DEC0, **kw)
    want = torch.stack([withbeam(case, fi, mode) for fi in range(len(FREQS))])
    assert torch.equal(got, want)
    # the beam is applied: the unbeamed predict is something else
    plain = ops.predict_coh_channels(pack, t.u, t.v, t.w, FREQS, S.FREQ0,
                                     S.FDELTA, S.TDELTA, S.DEC0)
    assert float((got - plain).abs().max()) > 0.1 * float(plain.abs().max())


def test_beamed_residuals_are_data_minus_beamed_model(case):
    pack, t, state, bb = (case[k] for k in ('pack', 'tile', 'state', 'bb'))
    got = ops.residuals_multifreq(
        pack, t.xo, t.u, t.v, t.w, FREQS, S.FREQ0, S.FDELTA, S.TDELTA,
        S.DEC0, state.J, chunk_table(state), bb[:45],
        subtract=[c >= 0 for c in pack.cluster_ids], beam=case['gains'],
        ejones=case['ej'])
    for fi in range(len(FREQS)):
        want = t.xo[fi] - sage.total_model(state, withbeam(case, fi, 2), bb,
                                           T, 45, skip={1})
        assert torch.equal(got[fi], want), fi


def test_sage_with_beam_on_the_cpu_is_the_coh_fn_loop(case, monkeypatch):
    pack, t, state, bb = (case[k] for k in ('pack', 'tile', 'state', 'bb'))
    calls = []

    def coh_fn(f):
        calls.append(f)
        return withbeam(case, FREQS.index(f), 2)

    def never(*a, **k):
        raise AssertionError("the CPU path must not call this")
    monkeypatch.setattr(ops, 'residuals_multifreq', never)
    loop = sage.calculate_residuals_multifreq(state, pack, t, bb,
                                              coh_fn=coh_fn)
    assert calls == list(FREQS)
    got = sage.calculate_residuals_multifreq(
        state, pack, t, bb, coh_fn=coh_fn,
        beam=dict(beam=case['gains'], ejones=case['ej']))
    assert calls == 2 * list(FREQS)
    assert torch.equal(got, loop)
    # a beam that nothing can apply is refused, not dropped
    with pytest.raises(ValueError):
        sage.calculate_residuals_multifreq(
            state, pack, t, bb, beam=dict(beam=case['gains']))
