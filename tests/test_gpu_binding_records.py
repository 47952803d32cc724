"""The two records of the extension's predict entry points, called directly:
`src` (GPUPack.record) and `tab` (ShapeletTable.record), dicts from field
name to tensor that bindings.cpp checks field by field.

Smallest shape with every field in use: 3 stations, 1 timeslot, R = 3 rows,
F = 2 channels; a 2-cluster pack of one point source each (K = 2) for `src`
and the one-shapelet pack of test_gpu_shapelet_channels.py (S = 1) for
`tab`. A broken record is refused by a check of the binding, before any
launch, so nothing here can fault."""
import pytest
import torch

import shapelet_sky as S
from test_gpu_shapelet_channels import SPECS
from sagecal_amd.ops import hip_host

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ARGS = (S.FREQ0, S.FDELTA, S.TDELTA, S.DEC0)
FREQS = [S.FREQ0, S.FREQ0 + 200e3]
R, M, K, NS = 3, 2, 2, 1


@pytest.fixture(scope='module')
def case():
    dev = torch.device(DEV)
    point = hip_host.gpu_pack(S.make_pack(spec=(), M=2, nsrc=1)[0], dev)
    one = hip_host.gpu_pack(S.make_pack(**SPECS['one'])[0], dev)
    assert (point.K, point.M, point.sh) == (K, M, None)
    assert (one.K, one.M, one.sh.S) == (K, M, NS)
    g = torch.Generator().manual_seed(5)
    cplx = lambda *s: torch.complex(torch.randn(*s, generator=g),
                                    torch.randn(*s, generator=g)).to(dev)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
    return dict(
        point=point, one=one,
        uvw=[t[:R].to(dev).contiguous() for t in S.uvw_rows()[:3]],
        x=cplx(len(FREQS), R, 2, 2), J=cplx(M, 3, 2, 2),
        chunk_tab=i32([[0], [1]]), pairs=i32([[0, 1], [0, 2], [1, 2]]))


def calls(case, gp, src=None, tab=None, flux=None):
    """The six entry points as closures over the pack gp, the records and
    the flux stack (default: the pack's own): name -> (call, out), out the
    tensor an in-place entry point adds into, else None."""
    ext = hip_host._ext()
    u, v, w = case['uvw']
    src = gp.record if src is None else src
    # per-call values from the public accessors of the pack, not from the
    # helper that hip_host's own calls go through
    stack, fq = gp.flux_stack(FREQS, S.FREQ0)
    r1 = gp.r1_for(S.DEC0)
    a = dict(src=(stack, r1), chan=(fq, S.FDELTA * 0.5, S.TDELTA))
    f1 = torch.stack(gp.fluxes_at(S.FREQ0, S.FREQ0))
    chan1 = (S.FREQ0, S.FDELTA * 0.5, S.TDELTA)
    mf_flux = stack if flux is None else flux
    res = (case['J'].reshape(M, 3, 4).contiguous(), case['chunk_tab'],
           case['pairs'], None)
    x4 = case['x'].reshape(len(FREQS), R, 4).contiguous()
    out = {
        'predict_coh': (lambda: ext.predict_coh(
            u, v, w, src, f1, r1, *chan1), None),
        'predict_coh_channels': (lambda: ext.predict_coh_channels(
            u, v, w, src, mf_flux, r1, *a['chan']), None),
        'residuals_multifreq': (lambda: ext.residuals_multifreq(
            x4, u, v, w, src, mf_flux, r1, *a['chan'], *res), None)}
    if gp.sh is not None:
        tab = gp.sh.record if tab is None else tab
        sh_stack = gp.shapelet_flux_stack(FREQS, S.FREQ0)
        sh_flux = sh_stack if flux is None else flux
        sf1 = gp.shapelet_fluxes_at(S.FREQ0, S.FREQ0)
        r1s = r1.index_select(0, gp.sh.src)
        o1 = ext.predict_coh(u, v, w, gp.record, f1, r1, *chan1)
        oF = ext.predict_coh_channels(u, v, w, gp.record, a['src'][0], r1,
                                      *a['chan'])
        oR = ext.residuals_multifreq(x4, u, v, w, gp.record, a['src'][0], r1,
                                     *a['chan'], *res)
        out.update({
            'shapelet_coh_add': (lambda: ext.shapelet_coh_add(
                o1, u, v, w, tab, sf1, r1s, *chan1), o1),
            'shapelet_coh_channels_add': (
                lambda: ext.shapelet_coh_channels_add(
                    oF, u, v, w, tab, sh_flux, r1s, *a['chan'], mean=False,
                    K=K), oF),
            'shapelet_residuals_add': (lambda: ext.shapelet_residuals_add(
                oR, u, v, w, tab, sh_flux, r1s, *a['chan'], *res, K=K), oR)})
    return out


def test_sound_records_are_accepted(case):
    F = len(FREQS)
    u, v, w = case['uvw']
    public = lambda gp, **kw: (
        hip_host.predict_coh_channels(gp, u, v, w, FREQS, *ARGS, **kw),
        hip_host.residuals_multifreq(gp, case['x'], u, v, w, FREQS, *ARGS,
                                     case['J'], case['chunk_tab'],
                                     case['pairs'], **kw))
    c = calls(case, case['point'])
    assert c['predict_coh'][0]().shape == (M, R, 4)
    coh, res = public(case['point'])
    got = c['predict_coh_channels'][0]()
    assert got.shape == (F, M, R, 4)
    assert torch.equal(got.view(F, M, R, 2, 2), coh)
    got = c['residuals_multifreq'][0]()
    assert got.shape == (F, R, 4) and torch.equal(got.view(F, R, 2, 2), res)

    c = calls(case, case['one'])
    coh, res = public(case['one'], shapelets=True)
    shapes = {'shapelet_coh_add': (M, R, 4),
              'shapelet_coh_channels_add': (F, M, R, 4),
              'shapelet_residuals_add': (F, R, 4)}
    for name, shape in shapes.items():
        call, out = c[name]
        before = out.clone()
        assert call() is None and out.shape == shape
        assert not torch.equal(out, before), name     # something was added
    assert torch.equal(
        c['shapelet_coh_channels_add'][1].view(F, M, R, 2, 2), coh)
    assert torch.equal(c['shapelet_residuals_add'][1].view(F, R, 2, 2), res)


def broken(rec, f32, i32, wide):
    """Every kind of broken copy of the record `rec`; f32 and i32 name one
    float32 and one int32 field of it, `wide` a field of more than one
    element (a strided view of one element is contiguous)."""
    t, tw = rec[f32], rec[wide]
    strided = torch.zeros(2 * tw.numel(), dtype=tw.dtype,
                          device=tw.device)[::2]
    assert strided.shape == tw.shape and not strided.is_contiguous()
    return {'missing key': {k: v for k, v in rec.items() if k != f32},
            'unknown key': dict(rec, bogus=t),
            'float64 for float32': dict(rec, **{f32: t.double()}),
            'int64 for int32': dict(rec, **{i32: rec[i32].long()}),
            'field on the CPU': dict(rec, **{f32: t.cpu()}),
            'strided field': dict(rec, **{wide: strided}),
            'short field': dict(rec, **{f32: t[:-1]})}


def refused(what, call, out):
    before = None if out is None else out.clone()
    with pytest.raises(RuntimeError):
        call()
        pytest.fail(f'{what} was accepted')
    assert out is None or torch.equal(out, before), what


def test_broken_records_are_refused(case):
    F = len(FREQS)
    gp = case['point']
    for what, rec in broken(gp.record, 'eX', 'stype', 'eX').items():
        c = calls(case, gp, src=rec)
        assert len(c) == 3
        for name in c if what == 'missing key' else ['predict_coh_channels']:
            refused(f'src, {what}, {name}', *c[name])
    flux = torch.ones(F + 1, 4, K, dtype=torch.float32, device=DEV)
    refused('src, flux [F + 1, 4, K]',
            *calls(case, gp, flux=flux)['predict_coh_channels'])
    gp = case['one']
    for what, rec in broken(gp.sh.record, 'beta', 'n0', 'coef').items():
        c = calls(case, gp, tab=rec)
        assert len(c) == 6
        for name in list(c)[3:] if what == 'missing key' \
                else ['shapelet_coh_channels_add']:
            refused(f'tab, {what}, {name}', *c[name])
    flux = torch.ones(F + 1, 4, NS, dtype=torch.float32, device=DEV)
    refused('tab, flux [F + 1, 4, S]',
            *calls(case, gp, flux=flux)['shapelet_coh_channels_add'])
