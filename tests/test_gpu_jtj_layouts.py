"""JtJ/Jtr assembly, cost and model kernels on station-pair tables the
data readers may hand over: pairs stored (q, p), tables in any row order,
chunks longer than one 64-lane pass, a station without baselines, and the
several-cluster residual. Every comparison is against reference.jtj_jtr /
reference.apply_jones in complex128 on the CPU, given the same bb.

Limits are those of test_gpu.py for these kernels: JtJ and Jtr
max|err|/max|ref| < 2e-5, per-chunk cost rtol 1e-5, apply_jones 5e-6."""
import numpy as np
import pytest
import torch

from sagecal_amd.ops import reference as R
from sagecal_amd.ops.hip_host import (BaselineLayout, apply_jones,
                                      model_cost_per_chunk, _ext, _c64)

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
JTJ_LIM = 2e-5
COST_RTOL = 1e-5
APPLY_LIM = 5e-6


def canonical(stations):
    s = list(stations)
    return np.array([(p, q) for i, p in enumerate(s) for q in s[i + 1:]])


def pair_table(name, N=6):
    """canonical: p < q, lexicographic. reversed: every pair stored (q, p).
    mixed: odd-numbered pairs reversed, rows in a fixed permutation."""
    t = canonical(range(N))
    if name == 'reversed':
        t = t[:, ::-1].copy()
    elif name == 'mixed':
        t[1::2] = t[1::2, ::-1]
        t = t[np.random.default_rng(1).permutation(len(t))]
    else:
        assert name == 'canonical'
    return t


def make_data(seed, B, nchunk, N):
    """x, coh [B,2,2] and J = I + 0.2 noise [nchunk,N,2,2] complex128,
    weights [B] uniform in [0.5, 2]."""
    rng = np.random.default_rng(seed)

    def cplx(*shape):
        return torch.tensor(rng.standard_normal(shape)
                            + 1j * rng.standard_normal(shape))
    x, coh = cplx(B, 2, 2), cplx(B, 2, 2)
    J = torch.tensor(np.eye(2)[None, None]) + 0.2 * cplx(nchunk, N, 2, 2)
    w = torch.tensor(rng.uniform(0.5, 2.0, B))
    return x, coh, J, w


def tiled(table, slots):
    return torch.tensor(np.tile(table, (slots, 1)))


def rows_of(chunk_tab, Nbase):
    return torch.tensor(np.repeat(np.asarray(chunk_tab), Nbase))


def run(bb, Nbase, T, nseg, N, rows, nchunk, data):
    """Kernel outputs (host, float64/complex128) next to their fp64
    references, for rows = seg*(T*Nbase) + t*Nbase + b with pair table
    bb[:Nbase] and per-row chunk ids `rows`."""
    x, coh, J, w = data
    JtJ_r, Jtr_r, _ = R.jtj_jtr(x, coh, J, bb, N, w, rows, nchunk)
    V_r = R.apply_jones(coh, J, bb, rows)
    e2 = w * ((x - V_r).abs() ** 2).sum(dim=(-1, -2))
    cost_r = torch.zeros(nchunk, dtype=torch.float64).index_add_(0, rows, e2)
    ref = dict(JtJ=JtJ_r, Jtr=Jtr_r, cost=cost_r, V=V_r)

    bbg, rg = bb.to(DEV), rows.to(DEV)
    lay = BaselineLayout(bbg, Nbase, T, nseg, N, DEV)
    xg = x.to(device=DEV, dtype=torch.complex64)
    cg = coh.to(device=DEV, dtype=torch.complex64)
    Jg = J.to(device=DEV, dtype=torch.complex64)
    wg = w.to(device=DEV, dtype=torch.float32)
    Jc = Jg.reshape(-1, 4).contiguous()
    ct = lay.chunk_tab(rg)
    JtJ, Jtr, cost = _ext().jtj_jtr(_c64(xg), _c64(cg), Jc, lay.pairs, ct,
                                    lay.pidx, wg, Nbase, T, N, nseg, nchunk)
    g, gcost = _ext().jtr_grad(_c64(xg), _c64(cg), Jc, lay.pairs, ct,
                               lay.pidx, wg, Nbase, T, N, nseg, nchunk)
    mc = model_cost_per_chunk(xg, cg, Jg, bbg, N, wg, rg, nchunk, lay)
    V = apply_jones(cg, Jg, bbg, rg, lay)
    got = dict(JtJ=JtJ, Jtr=Jtr, cost=cost, mc=mc, gcost=gcost,
               grad=torch.view_as_real(g).reshape(nchunk, 8 * N), V=V)
    return got, ref


def relerr(a, b):
    a = a.detach().cpu().to(b.dtype)
    return float((a - b).abs().max() / b.abs().max())


def asymmetry(JtJ, N):
    """max |JtJ - JtJ^T| over the diagonal 8x8 blocks and over the rest."""
    d = (JtJ - JtJ.transpose(1, 2)).abs().cpu()
    blk = torch.block_diag(*[torch.ones(8, 8)] * N).bool()
    return float(d[:, blk].max()), float(d[:, ~blk].max())


def check(got, ref, N, label, other=None):
    """Print the error figures, then hold them to the limits. `other`
    replaces the reference by another kernel run's outputs for JtJ, Jtr
    and cost (same limits)."""
    ref = dict(ref)
    if other is not None:
        for k in ('JtJ', 'Jtr', 'cost'):
            ref[k] = other[k].detach().cpu().double()
    errs = dict(JtJ=relerr(got['JtJ'], ref['JtJ']),
                Jtr=relerr(got['Jtr'], ref['Jtr']),
                grad=relerr(got['grad'], ref['Jtr']),
                V=relerr(got['V'], ref['V']))
    cost = {k: float(((got[k].cpu().double() - ref['cost']).abs()
                      / ref['cost'].abs()).max())
            for k in ('cost', 'mc', 'gcost')}
    asym = asymmetry(got['JtJ'], N)
    print(f"{label}: JtJ {errs['JtJ']:.2e} Jtr {errs['Jtr']:.2e} "
          f"jtr_grad {errs['grad']:.2e} apply_jones {errs['V']:.2e} "
          f"cost rel: jtj_jtr {cost['cost']:.2e} model_cost "
          f"{cost['mc']:.2e} jtr_grad {cost['gcost']:.2e}; "
          f"|JtJ - JtJ^T| diag blocks {asym[0]:.2e} others {asym[1]:.2e}")
    assert errs['JtJ'] < JTJ_LIM, errs
    assert errs['Jtr'] < JTJ_LIM, errs
    assert errs['grad'] < JTJ_LIM, errs
    assert errs['V'] < APPLY_LIM, errs
    for k in ('cost', 'mc', 'gcost'):
        assert torch.allclose(got[k].cpu().double(), ref['cost'],
                              rtol=COST_RTOL), (k, cost)
    assert torch.equal(got['JtJ'], got['JtJ'].transpose(1, 2)), asym
    assert all(bool(torch.isfinite(v).all()) for v in got.values()
               if not v.is_complex())


# ---- pair-table orders: N=6, all 15 pairs, T=4, 2 chunks [0,0,1,1] -------

ORD = dict(N=6, Nbase=15, T=4, nseg=1, nchunk=2)
ORD_ROWS = rows_of([0, 0, 1, 1], 15)


def order_data():
    return make_data(41, 4 * 15, 2, 6)


def run_order(name, data=None):
    bb = tiled(pair_table(name), ORD['T'])
    return run(bb, ORD['Nbase'], ORD['T'], ORD['nseg'], ORD['N'], ORD_ROWS,
               ORD['nchunk'], data or order_data())


@pytest.mark.parametrize('name', ('canonical', 'reversed', 'mixed'))
def test_pair_table_order(name):
    got, ref = run_order(name)
    check(got, ref, 6, name)


def test_orders_in_one_process():
    """canonical, mixed, canonical again: the second and third layouts
    meet a pair-index cache that another table of the same (N, Nbase)
    filled."""
    for name in ('canonical', 'mixed', 'canonical'):
        got, ref = run_order(name)
        check(got, ref, 6, 'sequence ' + name)


def test_reversed_table_is_the_same_visibilities():
    """Pair (q, p) with x^H and coh^H is pair (p, q) with x and coh: the
    kernel's JtJ, Jtr and cost must not depend on which way the table
    stores the pairs. No reference in this comparison."""
    x, coh, J, w = order_data()
    canon, _ = run_order('canonical', (x, coh, J, w))
    xh = x.conj().transpose(-1, -2).contiguous()
    ch = coh.conj().transpose(-1, -2).contiguous()
    got, ref = run_order('reversed', (xh, ch, J, w))
    check(got, ref, 6, 'reversed+hermitian vs canonical kernel run',
          other=canon)


# ---- chunks longer than one 64-lane pass ---------------------------------

def test_chunks_longer_than_a_wave():
    """N=4, T=129, two segments. Segment 0: chunk 0 = slots 0..63 (one
    pass exactly), chunk 1 = slots 64..128 (a pass plus one). Segment 1:
    chunk 2 = all 129 slots (two passes plus one). A second call returns
    bitwise the same."""
    N, T, nseg, nchunk = 4, 129, 2, 3
    table = canonical(range(N))
    Nbase = len(table)
    bb = tiled(table, nseg * T)
    rows = rows_of([0] * 64 + [1] * 65 + [2] * 129, Nbase)
    data = make_data(42, nseg * T * Nbase, nchunk, N)
    got, ref = run(bb, Nbase, T, nseg, N, rows, nchunk, data)
    check(got, ref, N, 'T=129')
    again, _ = run(bb, Nbase, T, nseg, N, rows, nchunk, data)
    for k in got:
        assert torch.equal(got[k], again[k]), k


# ---- a station with no baselines -----------------------------------------

def test_station_without_baselines():
    """N=5 with pairs over stations {0,1,2,4}: station 3's rows and
    columns of JtJ and entries of Jtr are exactly zero."""
    N, T = 5, 3
    table = canonical((0, 1, 2, 4))
    Nbase = len(table)
    bb = tiled(table, T)
    rows = rows_of([0] * T, Nbase)
    got, ref = run(bb, Nbase, T, 1, N, rows, 1,
                   make_data(43, T * Nbase, 1, N))
    check(got, ref, N, 'station 3 absent')
    assert float(got['JtJ'][:, 24:32, :].abs().max()) == 0.0
    assert float(got['JtJ'][:, :, 24:32].abs().max()) == 0.0
    assert float(got['Jtr'][:, 24:32].abs().max()) == 0.0
    assert float(got['grad'][:, 24:32].abs().max()) == 0.0
    assert float(ref['JtJ'][:, 24:32, :].abs().max()) == 0.0


# ---- k_apply_jones with several clusters ---------------------------------

def test_apply_jones_clusters_residual():
    """M=3 clusters with 1, 2 and 4 chunks (global chunk ids, tables
    stacked [M, T]) on the mixed table with one flagged pair:
    sub=1 gives x - sum_ci J_p C_ci J_q^H, sub=0 the sum; the flagged
    pair's rows come back as x and as zero."""
    N, T, M, Mt = 6, 4, 3, 7
    table = pair_table('mixed')
    Nbase = len(table)
    B = T * Nbase
    flagged = 4
    ftable = table.copy()
    ftable[flagged] = -1
    bb = tiled(table, T)
    tabs = np.array([[0, 0, 0, 0], [1, 1, 2, 2], [3, 4, 5, 6]])
    rng = np.random.default_rng(44)

    def cplx(*shape):
        return torch.tensor(rng.standard_normal(shape)
                            + 1j * rng.standard_normal(shape))
    x, cohs = cplx(B, 2, 2), cplx(M, B, 2, 2)
    J = torch.tensor(np.eye(2)[None, None]) + 0.2 * cplx(Mt, N, 2, 2)
    Vsum = sum(R.apply_jones(cohs[ci], J, bb, rows_of(tabs[ci], Nbase))
               for ci in range(M))
    frows = torch.arange(B) % Nbase == flagged
    want1 = torch.where(frows[:, None, None], x, x - Vsum)
    want0 = torch.where(frows[:, None, None], torch.zeros_like(x), Vsum)

    pairs = torch.tensor(ftable, dtype=torch.int32, device=DEV).contiguous()
    ct = torch.tensor(tabs.reshape(-1), dtype=torch.int32, device=DEV)
    xg = _c64(x.to(DEV))
    cg = cohs.to(device=DEV, dtype=torch.complex64).reshape(
        M * B, 4).contiguous()
    Jc = J.to(device=DEV, dtype=torch.complex64).reshape(-1, 4).contiguous()
    out1 = _ext().apply_jones(xg, cg, Jc, pairs, ct, Nbase, T, N, 1, M, 1)
    out0 = _ext().apply_jones(None, cg, Jc, pairs, ct, Nbase, T, N, 1, M, 0)
    out1 = out1.cpu().to(torch.complex128).view(B, 2, 2)
    out0 = out0.cpu().to(torch.complex128).view(B, 2, 2)
    e1 = float((out1 - want1).abs().max() / x.abs().max())
    e0 = float((out0 - want0).abs().max() / Vsum.abs().max())
    print(f"apply_jones M=3: sub=1 {e1:.2e} of max|x|, "
          f"sub=0 {e0:.2e} of max|sum V|")
    assert e1 < APPLY_LIM, e1
    assert e0 < APPLY_LIM, e0
    assert torch.equal(out1[frows], xg.cpu().to(torch.complex128)
                       .view(B, 2, 2)[frows])
    assert float(out0[frows].abs().max()) == 0.0
