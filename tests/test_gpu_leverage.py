"""ops.leverage_rows (k_leverage, leverage.hip) on the device against the
torch formula of solvers/diagnostics.py (_lin_blocks, _anti_blocks, the three
traces, blocks of Hinv indexed per row) in float64 on the CPU, from the same
complex64 draws and the same Hinv = inv(JtJ + MU I); then the kernel path of
diagnostics.leverage and influence_map(cluster=None).

MU = 1e-2 keeps sum |products| of a row, tr(|D1| |Hpp| |D1|^T) + ..., within
1390 x lev on the CPU reference for every case below (390 to 1390; the
bound asked for is 1e4), so 1e-9 * max(lev) covers some 300 float64 products
per row in another order, 300 x 2.2e-16 x 1e4, with a margin of about 1000.
Measured on an MI355X: max |lev - ref| 0.8e-13 to 1.4e-13 over the five
cases, max(lev) 1.9 to 3.4.

Through diagnostics.leverage at mu = 1e-6 (N = 8, T = 4, 2 chunks, max lev
2.88), against the complex128 CPU result, max |a - ref| measured on an
MI355X: kernel path 1.25e-07, torch path on the device
(SAGECAL_FORCE_REFERENCE=1) 4.69e-03 and 3.40e-03 in two runs (its
index_add has no fixed order). The kernel path may be 4 x the torch
path's error off, which allows for the float32 JtJ assembly that both share
(the rule of test_gpu_rtr_tcg.py). influence_map(cluster=None) against
cluster=ci: 0 for every cluster of the state below."""
import functools
import types

import numpy as np
import pytest
import torch

from sagecal_amd.ops import dispatch as ops
from sagecal_amd.ops import hip_host
from sagecal_amd.ops import reference as R
from sagecal_amd.solvers import diagnostics as diag
from sagecal_amd.solvers import sage

gpu = pytest.mark.gpu
DEV = 'cuda:0'
MU = 1e-2


@functools.lru_cache(maxsize=None)
def make(N, T, nchunks, odd_pairs=False, weighted=False, seed=5):
    """Seeded (cohs [M, R, 2, 2] c64, J [Mt, N, 2, 2] c64, Hinv f64,
    chunk_tab, pairs, weights or None) on the CPU, the reference lev [M, R]
    and the largest sum |products| / lev of a row. odd_pairs: shuffled, every
    third pair as (q, p), pair 1 repeating pair 0 and pair 2 flagged."""
    rng = np.random.default_rng(seed)

    def c64(*shape):
        return torch.tensor(rng.standard_normal(shape)
                            + 1j * rng.standard_normal(shape)
                            ).to(torch.complex64)
    pr = np.array([(p, q) for p in range(N) for q in range(p + 1, N)])
    if odd_pairs:
        pr = pr[rng.permutation(len(pr))]
        pr[::3] = pr[::3, ::-1]
        pr[1] = pr[0]
        pr[2] = (-1, pr[2, 1])
    Nbase, M, Mt = len(pr), len(nchunks), sum(nchunks)
    off = [sum(nchunks[:ci]) for ci in range(M)]
    tab = ops.lbfgs_chunk_table(off, nchunks, T, 'cpu')
    cohs = c64(M, T * Nbase, 2, 2)
    J = (torch.eye(2) + 0.2 * c64(Mt, N, 2, 2)).to(torch.complex64)
    w = torch.tensor(rng.uniform(0.5, 2.0, T * Nbase)) if weighted else None
    bb = torch.tensor(pr).repeat(T, 1)
    live = (bb >= 0).all(dim=1)
    Jd, bbc = J.to(torch.complex128), bb.clamp_min(0)
    Hinv, lev, cond = [], [], 0.0
    for ci in range(M):
        rows = tab[ci].long().repeat_interleave(Nbase) - off[ci]
        Jc, C = Jd[off[ci]:off[ci] + nchunks[ci]], cohs[ci].to(Jd.dtype)
        JtJ = R.jtj_jtr(C, C, Jc, bbc, N, live.double(), rows, nchunks[ci])[0]
        Hi = torch.linalg.inv(JtJ + MU * torch.eye(8 * N, dtype=JtJ.dtype))
        Hinv.append(Hi)
        D1 = diag._lin_blocks(C @ Jc[rows, bbc[:, 1]].conj().transpose(-1, -2))
        D2 = diag._anti_blocks(Jc[rows, bbc[:, 0]] @ C)
        H5 = Hi.reshape(-1, N, 8, N, 8)
        blk = lambda a, b: H5[rows, bbc[:, a], :, bbc[:, b], :]

        def traces(D1, D2, Hpp, Hqq, Hpq):
            t = (D1 @ Hpp @ D1.mT + D2 @ Hqq @ D2.mT + 2 * (D1 @ Hpq @ D2.mT))
            return t.diagonal(dim1=-2, dim2=-1).sum(-1)
        H3 = blk(0, 0), blk(1, 1), blk(0, 1)
        lv = traces(D1, D2, *H3)
        cond = max(cond, float((traces(D1.abs(), D2.abs(),
                                       *(h.abs() for h in H3)) / lv)[live]
                               .max()))
        lev.append(torch.where(live, lv, 0.0) * (1.0 if w is None else w))
    pairs = torch.tensor(pr, dtype=torch.int32)
    return ((cohs, J, torch.cat(Hinv), tab, pairs, w), torch.stack(lev), cond)


CASES = {
    'below_a_wave': (3, 4, (1,)),
    'tile_boundary_uneven_chunks': (12, 5, (2, 1)),
    'odd_pair_table': (6, 3, (1, 1, 1), True),
    'weights': (12, 5, (2, 1), False, True),
    'one_timeslot_per_piece': (12, 7, (7,)),
}


@gpu
@pytest.mark.parametrize('case', CASES)
def test_op_against_formula(case):
    inp, ref, cond = make(*CASES[case])
    assert cond <= 1e4, cond
    dev = [None if t is None else t.to(DEV) for t in inp]
    out = ops.leverage_rows(*dev)
    assert torch.equal(out, ops.leverage_rows(*dev))    # bit for bit
    assert out.dtype == torch.float64 and out.shape == ref.shape
    err = float((out.cpu() - ref).abs().max())
    print(f'{case}: max lev {float(ref.max()):.3f} cond {cond:.1f} '
          f'err {err:.2e} limit {1e-9 * float(ref.max()):.2e}')
    assert err <= 1e-9 * float(ref.max())
    if case == 'odd_pair_table':                        # the flagged pair
        assert not out[:, 2::inp[4].shape[0]].any()


def test_cpu_formula_per_chunk_and_pair():
    """The torch implementation off the device, blocks per (chunk, pair)."""
    for case in ('tile_boundary_uneven_chunks', 'odd_pair_table', 'weights'):
        inp, ref, _ = make(*CASES[case])
        err = float((ops.leverage_rows(*inp) - ref).abs().max())
        assert err <= 1e-9 * float(ref.max())


def solve_inputs(N, T, nchunks, seed=9):
    """x = model of a known J plus noise, cohs, bb and a state 5 % off."""
    rng = np.random.default_rng(seed)
    cplx = lambda *s: torch.tensor(rng.standard_normal(s)
                                   + 1j * rng.standard_normal(s))
    pr = [(p, q) for p in range(N) for q in range(p + 1, N)]
    Nbase, bb = len(pr), torch.tensor(pr * T)
    M = len(nchunks)
    state = sage.CalState(types.SimpleNamespace(M=M, nchunk=list(nchunks)), N)
    cohs = cplx(M, T * Nbase, 2, 2)
    Jt = state.J + 0.2 * cplx(*state.J.shape)
    x = 0.01 * cplx(T * Nbase, 2, 2)
    for ci in range(M):
        o = state.chunk_off[ci]
        x = x + R.apply_jones(cohs[ci], Jt[o:o + nchunks[ci]], bb,
                              R.chunk_rows_for(ci, nchunks, T, Nbase,
                                               T * Nbase, 'cpu'))
    state.J = (Jt + 0.05 * cplx(*Jt.shape)).to(torch.complex64)
    tile = types.SimpleNamespace(tilesz=T, Nbase=Nbase,
                                 x=x.to(torch.complex64))
    return state, cohs.to(torch.complex64), tile, bb


@gpu
def test_through_diagnostics_leverage(monkeypatch):
    N, T = 8, 4
    state, cohs, tile, bb = solve_inputs(N, T, (2,))
    Nbase = tile.Nbase
    rows = R.chunk_rows_for(0, state.nchunks, T, Nbase, T * Nbase, 'cpu')
    c128 = lambda t: t.to(torch.complex128)
    ref = diag.leverage(c128(tile.x), c128(cohs[0]), c128(state.J), bb, N,
                        chunk_rows=rows, nchunk=2, mu=1e-6)
    bbd = bb.to(DEV)
    args = (tile.x.to(DEV), cohs[0].to(DEV), state.J.to(DEV), bbd, N)
    kw = dict(chunk_rows=rows.to(DEV), nchunk=2, mu=1e-6, T=T, Nbase=Nbase,
              layout=hip_host.BaselineLayout(bbd, Nbase, T, 1, N, DEV))
    calls = []
    real = hip_host.leverage_rows
    monkeypatch.setattr(hip_host, 'leverage_rows',
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    kern = diag.leverage(*args, **kw).cpu()
    assert len(calls) == 1
    monkeypatch.setenv('SAGECAL_FORCE_REFERENCE', '1')
    ref_dev = diag.leverage(*args, **kw).cpu()
    assert len(calls) == 1
    e_kern = float((kern - ref).abs().max())
    e_torch = float((ref_dev - ref).abs().max())
    print(f'max lev {float(ref.max()):.3f}: kernel path {e_kern:.2e}, torch '
          f'device path {e_torch:.2e}')
    assert e_kern <= 4 * e_torch
    assert float(kern.min()) >= 0.0
    assert float(kern.max()) <= 8.0 + 4 * e_torch


@gpu
def test_influence_map_all_clusters():
    """Every cluster has at least two chunks: torch.linalg.inv of a single
    matrix takes another routine than the batched one, and at mu = 1e-6 its
    result moved lev by 7.0e-10 (measured, a cluster of one chunk), more than
    half of the limit, for a reason that is not the kernel's."""
    state, cohs, tile, bb = solve_inputs(6, 6, (2, 3, 2))
    state.J, tile.x, cohs, bb = (t.to(DEV)
                                 for t in (state.J, tile.x, cohs, bb))
    every = diag.influence_map(state, cohs, tile, bb, cluster=None)
    assert every.shape == (3, tile.x.shape[0])
    for ci in range(3):
        one = diag.influence_map(state, cohs, tile, bb, cluster=ci)
        err = float((every[ci] - one).abs().max())
        print(f'cluster {ci}: max lev {float(one.max()):.3f} err {err:.2e}')
        assert err <= 1e-9 * float(one.max())
