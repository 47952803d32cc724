"""ops.joint_jtj_jtr and ops.joint_cost (joint_jtj.hip) in complex64 on the
device against reference.joint_jtj_jtr in complex128 on the CPU from the same
inputs, and lm.joint_lm_solve with SAGECAL_JOINT_KERNEL=1 against the
switch-off path.

Limits are test_gpu.py::test_jtj_jtr_matches_reference's: max|H - H_ref| /
max|H_ref| < 2e-5, the same for g, cost rel 1e-4. Largest measured on an
MI355X over the cases below: H 1.2e-07, g 1.3e-07, cost 5.7e-08, trial cost
4.5e-08. Solver, from identity, 12 iterations, initial cost 2.12e+02: final
cost 6.2e-12 with the switch off, 4.2e-12 with it on."""
import numpy as np
import pytest
import torch

from sagecal_amd.ops import dispatch as ops
from sagecal_amd.ops import hip_host
from sagecal_amd.ops import reference as R
from sagecal_amd.solvers import lm

gpu = pytest.mark.gpu
DEV = 'cuda:0'
LIM, COST_REL = 2e-5, 1e-4
TILE1 = hip_host.JOINT_TT + 1           # one timeslot past the time tile


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


def make_data(seed, M, Mt, R_, N):
    """x [R,2,2], cohs [M,R,2,2], J = I + 0.2 noise [Mt,N,2,2], weights [R]
    in (0.5, 1.5); complex128 / float64."""
    rng = np.random.default_rng(seed)

    def cplx(*shape):
        return torch.tensor(rng.standard_normal(shape)
                            + 1j * rng.standard_normal(shape))
    return (cplx(R_, 2, 2), cplx(M, R_, 2, 2),
            torch.tensor(np.eye(2)[None, None]) + 0.2 * cplx(Mt, N, 2, 2),
            torch.tensor(0.5 + rng.random(R_)))


def blocks(H, g, M, Kb, N):
    """Diagonal blocks [Kb, Pb, Pb], [Kb, Pb] of the dense result: block k
    holds chunk k of every cluster, order (cluster, station, 8)."""
    H6 = H.reshape(M, Kb, N * 8, M, Kb, N * 8)
    Hb = torch.stack([H6[:, k, :, :, k, :].reshape(M * N * 8, -1)
                      for k in range(Kb)])
    return Hb, g.reshape(M, Kb, N * 8).transpose(0, 1).reshape(Kb, -1)


def make_case(N, T, nchunks, table, weighted, blocked, flagged, stations,
              on_gpu=True):
    """(reference inputs, device inputs) of one case; the reference gets a
    flagged pair's rows as x = coh = 0 on pair (0, 1)."""
    tab = pair_table(table, stations or range(N))
    Nbase, M, Mt = len(tab), len(nchunks), sum(nchunks)
    chunk_off = np.cumsum([0] + nchunks[:-1]).tolist()
    x, cohs, J, w = make_data(7, M, Mt, T * Nbase, N)
    w = w if weighted else None
    xr, cr, ref_tab, gpu_tab = x, cohs, tab.copy(), tab.copy()
    if flagged is not None:
        rows = torch.arange(T * Nbase) % Nbase == flagged
        xr, cr = x.clone(), cohs.clone()
        xr[rows], cr[:, rows] = 0, 0
        ref_tab[flagged], gpu_tab[flagged] = (0, 1), (-1, -1)
    rest = (chunk_off, nchunks)
    ref = (xr, cr, J, *rest, torch.tensor(np.tile(ref_tab, (T, 1))), T,
           Nbase, w)
    if not on_gpu:
        return ref, None
    dev = (x.to(DEV, torch.complex64), cohs.to(DEV, torch.complex64),
           J.to(DEV, torch.complex64), *rest,
           torch.tensor(np.tile(gpu_tab, (T, 1)), device=DEV), T, Nbase,
           None if w is None else w.to(DEV, torch.float32))
    return ref, dev


def ref_block_costs(ref, Kb):
    """The cost R.joint_jtj_jtr returns with the rows outside block k
    weighted 0, for every k."""
    *head, T, Nbase, w = ref
    k_row = R.chunk_rows_for(0, [Kb], T, Nbase, T * Nbase, 'cpu')
    k_row = torch.zeros(T * Nbase) if k_row is None else k_row
    w = torch.ones(T * Nbase, dtype=torch.float64) if w is None else w
    return torch.stack([R.joint_jtj_jtr(*head, T, Nbase, w * (k_row == k))[2]
                        for k in range(Kb)])


def rel(a, b):
    return float((a.cpu().double() - b).abs().max() / b.abs().max())


# N, T, nchunks, pair table, weights, blocked, flagged pair, stations
CASES = [
    (3, 2, [1, 2], 'canonical', False, False, None, None),
    (5, 5, [1, 2, 3], 'mixed', True, False, None, None),
    (12, 5, [1, 2, 3], 'reversed', False, False, None, None),   # 66 pairs
    (5, 5, [2, 2, 2], 'canonical', True, True, None, None),     # chunks 3 + 2
    (5, 5, [1] * 5, 'mixed', False, True, None, None),          # 8 M = 40
    (5, 5, [1], 'canonical', False, False, None, None),         # M = 1
    (5, TILE1, [1, 1], 'reversed', False, False, None, None),   # tile + 1
    (12, 5, [1, 2, 3], 'mixed', False, False, 4, None),         # flagged pair
    (5, 5, [1, 2, 3], 'canonical', False, False, None, (0, 1, 2, 4)),
]


@gpu
@pytest.mark.parametrize(
    'N,T,nchunks,table,weighted,blocked,flagged,stations', CASES)
def test_against_reference(N, T, nchunks, table, weighted, blocked, flagged,
                           stations):
    ref, dev = make_case(N, T, nchunks, table, weighted, blocked, flagged,
                         stations)
    H_ref, g_ref, c_ref = R.joint_jtj_jtr(*ref)
    if blocked:
        H_ref, g_ref = blocks(H_ref, g_ref, len(nchunks), nchunks[0], N)
        c_ref = ref_block_costs(ref, nchunks[0])
    H, g, c = ops.joint_jtj_jtr(*dev, blocked=blocked)
    assert H.shape == H_ref.shape and g.shape == g_ref.shape
    eh, eg = rel(H, H_ref), rel(g, g_ref)
    ec = float((c.cpu().double() / c_ref - 1).abs().max())
    print(f'N={N} T={T} {nchunks} {table}: H {eh:.2e} g {eg:.2e} '
          f'cost {ec:.2e}')
    assert eh < LIM and eg < LIM and ec < COST_REL
    again = ops.joint_jtj_jtr(*dev, blocked=blocked)
    assert all(torch.equal(a, b) for a, b in zip((H, g, c), again))
    if not blocked:
        assert torch.equal(H, H.T)
    if stations:
        Mt = sum(nchunks)
        H5 = H.view(Mt, N, 8, Mt, N, 8)
        assert float(H5[:, 3].abs().max()) == 0.0
        assert float(H5[:, :, :, :, 3].abs().max()) == 0.0
        assert float(g.view(Mt, N, 8)[:, 3].abs().max()) == 0.0


@gpu
@pytest.mark.parametrize('case', (1, 3))
def test_cost_only(case):
    blocked = CASES[case][5]
    ref, dev = make_case(*CASES[case])
    rng = torch.Generator().manual_seed(5)
    dJ = 0.05 * torch.randn(ref[2].shape, dtype=torch.complex128,
                            generator=rng)
    ref = ref[:2] + (ref[2] + dJ,) + ref[3:]
    dev = dev[:2] + (dev[2] + dJ.to(DEV, torch.complex64),) + dev[3:]
    c_ref = ref_block_costs(ref, CASES[case][2][0]) if blocked \
        else R.joint_jtj_jtr(*ref)[2]
    c = ops.joint_cost(*dev, blocked=blocked)
    ec = float((c.cpu().double() / c_ref - 1).abs().max())
    print(f'case {case}: trial cost rel {ec:.2e}')
    assert c.shape == c_ref.shape and ec < COST_REL


@gpu
def test_solver_switch(monkeypatch):
    N, T, nchunks = 5, 4, [2, 2]
    tab = pair_table('canonical', range(N))
    Nbase = len(tab)
    _, cohs, Jt, _ = make_data(11, 2, 4, T * Nbase, N)
    bb = torch.tensor(np.tile(tab, (T, 1)))
    x = sum(R.apply_jones(cohs[ci], Jt[2 * ci:2 * ci + 2], bb,
                          R.chunk_rows_for(ci, nchunks, T, Nbase, T * Nbase,
                                           'cpu')) for ci in range(2))
    J0 = torch.eye(2, dtype=torch.complex64, device=DEV).expand(
        4, N, 2, 2).contiguous()
    args = (x.to(DEV, torch.complex64), cohs.to(DEV, torch.complex64), J0,
            [0, 2], nchunks, bb.to(DEV), T, Nbase)
    init = float(ops.joint_cost(*args))
    _, off = lm.joint_lm_solve(*args, maxiter=12)
    calls = []
    real = hip_host.joint_jtj_jtr
    monkeypatch.setattr(hip_host, 'joint_jtj_jtr',
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setenv('SAGECAL_JOINT_KERNEL', '1')
    _, on = lm.joint_lm_solve(*args, maxiter=12)
    print(f'initial {init:.4e} switch off {off:.4e} switch on {on:.4e}')
    assert len(calls) > 0
    assert on <= 2 * off and on < 1e-6 * init


def test_blocked_on_cpu_matches_dense_blocks():
    ref, _ = make_case(5, 5, [2, 2, 2], 'mixed', True, True, None, None,
                        on_gpu=False)
    H, g, c = R.joint_jtj_jtr(*ref)
    Hb_ref, gb_ref = blocks(H, g, 3, 2, 5)
    Hb, gb, cb = ops.joint_jtj_jtr(*ref, blocked=True)
    assert torch.equal(Hb, Hb_ref) and torch.equal(gb, gb_ref)
    assert float(cb.sum()) == pytest.approx(float(c), rel=1e-12)
    torch.testing.assert_close(ops.joint_cost(*ref, blocked=True), cb)
    torch.testing.assert_close(cb, ref_block_costs(ref, 2))


def test_blocked_needs_uniform_chunks():
    ref, _ = make_case(5, 5, [1, 2, 3], 'canonical', False, False, None,
                        None, on_gpu=False)
    with pytest.raises(ValueError):
        ops.joint_jtj_jtr(*ref, blocked=True)
    with pytest.raises(ValueError):
        ops.joint_cost(*ref, blocked=True)
