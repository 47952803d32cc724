"""ops.lbfgs_cost_grad_channels (lbfgs_mf.hip) against the sum over the
channels of reference.lbfgs_cost_grad in complex128 on the CPU, from the same
inputs, and the SAGECAL_LBFGS_CHANNELS=1 routes against the switch-off path.

Limits are test_gpu.py::test_lbfgs_cost_grad_gpu's: cost rel 2e-4, gradient
max|err| / max|g_ref| < 1e-4. Largest measured on an MI355X over the cases
below: cost 6.2e-08 and gradient 1.3e-07 against the reference, gradient
1.8e-07 against the switch-off path."""
import numpy as np
import pytest
import torch

from sagecal_amd.ops import dispatch as ops
from sagecal_amd.ops import hip_host
from sagecal_amd.ops import reference as R
from sagecal_amd.solvers import stochastic

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
COST_REL, GRAD_LIM = 2e-4, 1e-4
SPLIT1 = hip_host.LBFGS_TSPLIT + 1      # one timeslot past the time split


def pair_table(name, stations):
    """canonical: p < q, lexicographic. reversed: every pair stored (q, p).
    mixed: odd-numbered pairs reversed, rows in a fixed permutation."""
    s = list(stations)
    t = np.array([(p, q) for i, p in enumerate(s) for q in s[i + 1:]])
    if name == 'reversed':
        t = t[:, ::-1].copy()
    elif name == 'mixed':
        t[1::2] = t[1::2, ::-1]
        t = t[np.random.default_rng(1).permutation(len(t))]
    return t


def make_data(seed, F, M, Mt, R_, N):
    """xs [F,R,2,2], cohs [F,M,R,2,2], J = I + 0.2 noise [Mt,N,2,2],
    complex128."""
    rng = np.random.default_rng(seed)

    def cplx(*shape):
        return torch.tensor(rng.standard_normal(shape)
                            + 1j * rng.standard_normal(shape))
    return (cplx(F, R_, 2, 2), cplx(F, M, R_, 2, 2),
            torch.tensor(np.eye(2)[None, None]) + 0.2 * cplx(Mt, N, 2, 2))


def c64(t):
    return t.to(device=DEV, dtype=torch.complex64)


def check(got, ref, label):
    (c, g), (c_ref, g_ref) = got, ref
    gerr = float((g.cpu().double() - g_ref).abs().max() / g_ref.abs().max())
    print(f'{label}: cost rel {abs(float(c) / float(c_ref) - 1):.2e} '
          f'grad {gerr:.2e}')
    assert float(c) == pytest.approx(float(c_ref), rel=COST_REL)
    assert gerr < GRAD_LIM, gerr


# N, T, nchunks, F, nu, pair table, flagged pair or None, stations
CASES = [
    (5, 5, [1, 2, 3], 1, None, 'canonical', None, None),    # under one wave
    (5, 5, [1, 2, 3], 3, 5.0, 'reversed', None, None),
    (12, 5, [1, 2, 3], 3, 5.0, 'mixed', None, None),        # 66 pairs
    (12, 5, [1, 2, 3], 1, None, 'reversed', None, None),
    (24, 2, [1, 2], 3, 5.0, 'mixed', None, None),           # 276: two tiles
    (5, SPLIT1, [1, 2], 1, 5.0, 'canonical', None, None),   # split plus one
    (12, SPLIT1, [1, 3], 3, None, 'mixed', None, None),
    (12, 5, [1, 2, 3], 3, 5.0, 'mixed', 4, None),           # flagged pair
    (5, 5, [1, 2, 3], 1, 5.0, 'canonical', None, (0, 1, 2, 4)),  # 3 absent
]


@pytest.mark.parametrize('N,T,nchunks,F,nu,table,flagged,stations', CASES)
def test_against_reference(N, T, nchunks, F, nu, table, flagged, stations):
    tab = pair_table(table, stations or range(N))
    Nbase, M, Mt = len(tab), len(nchunks), sum(nchunks)
    chunk_off = np.cumsum([0] + nchunks[:-1]).tolist()
    xs, cohs, J = make_data(7, F, M, Mt, T * Nbase, N)
    ref_tab, gpu_tab = tab.copy(), tab.copy()
    if flagged is not None:
        # the reference gets these rows as x = coh = 0 on pair (0, 1)
        rows = torch.arange(T * Nbase) % Nbase == flagged
        xr, cr = xs.clone(), cohs.clone()
        xr[:, rows], cr[:, :, rows] = 0, 0
        ref_tab[flagged], gpu_tab[flagged] = (0, 1), (-1, -1)
    else:
        xr, cr = xs, cohs
    bb = torch.tensor(np.tile(ref_tab, (T, 1)))
    ref = [R.lbfgs_cost_grad(xr[f], cr[f], J, chunk_off, nchunks, bb, T,
                             Nbase, robust_nu=nu) for f in range(F)]
    ref = sum(c for c, _ in ref), sum(g for _, g in ref)
    args = (c64(xs), c64(cohs), c64(J),
            ops.lbfgs_chunk_table(chunk_off, nchunks, T, DEV),
            torch.tensor(gpu_tab, dtype=torch.int32, device=DEV), nu)
    got = ops.lbfgs_cost_grad_channels(*args)
    check(got, ref, f'N={N} T={T} F={F} nu={nu} {table}')
    again = ops.lbfgs_cost_grad_channels(*args)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])
    if stations:
        absent = got[1].view(Mt, N, 8)[:, 3]
        assert float(absent.abs().max()) == 0.0


def switch_case():
    N, T, nchunks, F = 12, 5, [1, 2, 3], 3
    tab = pair_table('mixed', range(N))
    xs, cohs, J = make_data(8, F, 3, 6, T * len(tab), N)
    bb = torch.tensor(np.tile(tab, (T, 1)), device=DEV)
    return c64(xs), c64(cohs), c64(J), [0, 1, 3], nchunks, bb, T, len(tab)


def test_switch_routes_lbfgs_cost_grad(monkeypatch):
    xs, cohs, J, *rest = switch_case()
    w = torch.rand(xs.shape[1], device=DEV)
    off = ops.lbfgs_cost_grad(xs[0], cohs[0], J, *rest, robust_nu=5.0)
    off_w = ops.lbfgs_cost_grad(xs[0], cohs[0], J, *rest, robust_nu=5.0,
                                weights=w)
    monkeypatch.setenv('SAGECAL_LBFGS_CHANNELS', '1')
    monkeypatch.setattr(hip_host, 'lbfgs_cost_grad', None)  # not reached
    on = ops.lbfgs_cost_grad(xs[0], cohs[0], J, *rest, robust_nu=5.0)
    check(on, (off[0].cpu().double(), off[1].cpu().double()), 'switch')
    monkeypatch.undo()
    monkeypatch.setenv('SAGECAL_LBFGS_CHANNELS', '1')
    on_w = ops.lbfgs_cost_grad(xs[0], cohs[0], J, *rest, robust_nu=5.0,
                               weights=w)
    assert torch.equal(on_w[0], off_w[0]) and torch.equal(on_w[1], off_w[1])


def test_switch_routes_band_multifreq(monkeypatch):
    xs, cohs, J, *rest = switch_case()
    Mt, N = J.shape[:2]
    v = torch.view_as_real(J).reshape(-1)
    g = torch.Generator().manual_seed(3)
    cons = (torch.randn(v.numel(), generator=g).to(DEV),
            torch.randn(v.numel(), generator=g).to(DEV), 1.5)

    def call():
        return stochastic._cost_grad_band_multifreq(
            v, xs, list(cohs), *rest, Mt, N, torch.complex64, 5.0,
            consensus=cons)
    off = call()
    monkeypatch.setenv('SAGECAL_LBFGS_CHANNELS', '1')
    monkeypatch.setattr(hip_host, 'lbfgs_cost_grad', None)  # not reached
    check(call(), (off[0].cpu().double(), off[1].cpu().double()), 'band')


@pytest.mark.parametrize('bad', ('chunk', 'pair'))
def test_tables_out_of_range(bad):
    xs, cohs, J, chunk_off, nchunks, bb, T, Nbase = switch_case()
    tab = ops.lbfgs_chunk_table(chunk_off, nchunks, T, DEV).clone()
    pairs = bb[:Nbase].to(torch.int32)
    if bad == 'chunk':
        tab[2, 4] = J.shape[0]
    else:
        pairs[3, 1] = J.shape[1]
    with pytest.raises(ValueError):
        ops.lbfgs_cost_grad_channels(xs, cohs, J, tab, pairs, 5.0)
