"""ops.normal_matrices (k_normal_accum and k_normal_expand, normal_f64.hip)
on the device against reference.jtj_jtr on complex128 upcasts of the same
complex64 draws, cluster by cluster; its invariants; the CPU path and the
argument checks; and influence_map(cluster=None) with the float64 assembly.

Limit 1e-11 * max |ref|: an entry sums fewer than 8 (N - 1) T <= 6e3
products of float32-exact inputs, in float64 at worst 6e3 x 1.1e-16 = 7e-13
of the entry scale. A float32 assembly sits near 1e-7. Measured on an
MI355X: 1.3e-16 to 1.1e-15 over the six cases; through influence_map 2.0e-9
against 7.8e-8 for the float32 assembly with torch.linalg.inv (max lev
1.79)."""
import functools

import pytest
import torch

from sagecal_amd.ops import dispatch as ops
from sagecal_amd.ops import reference as R
from sagecal_amd.solvers import diagnostics as diag
from test_gpu_leverage import make, solve_inputs

gpu = pytest.mark.gpu
DEV = 'cuda:0'

CASES = {                                 # N, T, chunks, weights, odd table
    'below_a_wave': (3, 1, (1,), False, False),
    'two_chunks': (8, 4, (2,), False, False),
    'second_pair_tile_uneven_runs': (12, 6, (1, 3), False, False),
    'pieces_and_boundary_at_35': (8, 70, (1, 2), False, False),
    'weights': (12, 6, (1, 3), True, False),
    'negative_and_missing_pair': (8, 4, (2,), False, True),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """((cohs, J, chunk_tab, pairs, weights) on the CPU, ref [Mt, 8N, 8N]).
    The odd table flags pair 2, stores every third pair as (q, p) and adds a
    station to J that no pair names."""
    N, T, nchunks, weighted, odd = CASES[name]
    cohs, J, _, tab, pairs, w = make(N, T, nchunks, False, weighted)[0]
    pairs = pairs.clone()
    if odd:
        pairs[::3] = pairs[::3].flip(1)
        pairs[2, 0] = -1
        J, N = torch.cat([J, J[:, :1] * 1.5], dim=1), N + 1
    w = None if w is None else w.float()
    bb = pairs.long().repeat(T, 1)
    wt = (bb >= 0).all(dim=1).double() * (1.0 if w is None else w.double())
    ref, off = [], 0
    for ci, nc in enumerate(nchunks):
        C = cohs[ci].to(torch.complex128)
        rows = tab[ci].long().repeat_interleave(len(pairs)) - off
        ref.append(R.jtj_jtr(C, C, J[off:off + nc].to(C.dtype),
                             bb.clamp_min(0), N, wt, rows, nc)[0])
        off += nc
    return (cohs, J, tab, pairs, w), torch.cat(ref)


def on_dev(inp):
    return [None if t is None else t.to(DEV) for t in inp]


@gpu
@pytest.mark.parametrize('name', CASES)
def test_against_complex128_reference(name):
    inp, ref = case(name)
    out = ops.normal_matrices(*on_dev(inp))
    assert out.dtype == torch.float64 and out.shape == ref.shape
    ratio = float((out.cpu() - ref).abs().max() / ref.abs().max())
    print(f'{name}: max |JtJ - ref| / max |ref| = {ratio:.2e}')
    assert ratio <= 1e-11


@gpu
def test_invariants():
    inp, _ = case('second_pair_tile_uneven_runs')
    cohs, J, tab, pairs, _ = on_dev(inp)
    out = ops.normal_matrices(cohs, J, tab, pairs)
    assert torch.equal(out, out.mT)
    assert torch.equal(out, ops.normal_matrices(cohs, J, tab, pairs))
    alone = ops.normal_matrices(cohs[1:], J, tab[1:], pairs)
    assert torch.equal(alone[1:], out[1:]) and not alone[0].any()


def test_cpu_path_and_argument_checks(monkeypatch):
    for name in ('weights', 'negative_and_missing_pair'):
        inp, ref = case(name)
        assert torch.allclose(ops.normal_matrices(*inp), ref, rtol=0,
                              atol=1e-13 * float(ref.abs().max()))
    cohs, J, tab, pairs, _ = case('two_chunks')[0]
    with pytest.raises(ValueError):
        ops.normal_matrices(cohs[:, :-1], J, tab, pairs)
    with pytest.raises(ValueError):
        ops.normal_matrices(cohs, J, tab.repeat(2, 1), pairs)
    monkeypatch.delenv('SAGECAL_FORCE_REFERENCE', raising=False)
    monkeypatch.delenv('SAGECAL_NORMAL_F64', raising=False)
    assert not ops.normal_f64_on()
    monkeypatch.setenv('SAGECAL_NORMAL_F64', '1')
    assert ops.normal_f64_on()
    monkeypatch.setenv('SAGECAL_FORCE_REFERENCE', '1')
    assert not ops.normal_f64_on()


@gpu
def test_through_influence_map(monkeypatch):
    """No chunk may go back to torch.linalg.inv, and the map may be no
    further from the complex128 CPU leverage than the parent's path is."""
    N, T, nchunks = 16, 6, (1, 3)
    state, cohs, tile, bb = solve_inputs(N, T, nchunks)
    c128 = lambda t: t.to(torch.complex128)
    ref = torch.stack([
        diag.leverage(c128(tile.x), c128(cohs[ci]),
                      c128(state.cluster_J(ci)), bb, N,
                      chunk_rows=R.chunk_rows_for(ci, nchunks, T, tile.Nbase,
                                                  len(bb), 'cpu'),
                      nchunk=nchunks[ci], mu=1e-6)
        for ci in range(len(nchunks))])
    state.J, tile.x, cohs, bb = (t.to(DEV)
                                 for t in (state.J, tile.x, cohs, bb))
    calls = []
    real = ops.spd_inverse_torch
    monkeypatch.setattr(ops, 'spd_inverse_torch',
                        lambda *a: calls.append(1) or real(*a))
    monkeypatch.setenv('SAGECAL_NORMAL_F64', '1')
    monkeypatch.setenv('SAGECAL_INVERSE_KERNEL', '1')
    new = diag.influence_map(state, cohs, tile, bb, cluster=None).cpu()
    assert len(calls) == 0
    monkeypatch.delenv('SAGECAL_NORMAL_F64')
    monkeypatch.delenv('SAGECAL_INVERSE_KERNEL')
    old = diag.influence_map(state, cohs, tile, bb, cluster=None).cpu()
    e_new = float((new - ref).abs().max())
    e_old = float((old - ref).abs().max())
    print(f'max lev {float(ref.max()):.3f}: float64 assembly and inverse '
          f'kernels {e_new:.2e}, float32 assembly and linalg.inv {e_old:.2e}')
    assert e_new <= e_old
