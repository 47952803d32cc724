"""The blocked Cholesky kernels (cholesky_blocked.hip, outer block X = 128)
against an fp64 host solve of the same fp32 inputs, A = G G^T / n + 0.5 I
with mu in [0.01, 1); error = max|dp - ref| / max|ref|."""
import numpy as np
import pytest
import torch

from sagecal_amd.ops import dispatch as ops
from sagecal_amd.ops import hip_host
from sagecal_amd.ops import reference as R
from sagecal_amd.solvers import lm

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
X = 128
LIM = 1e-3              # the limit of test_gpu.py for this family
LIM_4104 = 4.6e-6       # see test_above_the_old_limit
JOINT_REL = 2.2e-6      # see test_joint_path


def problem(n, batch, seed):
    """fp32 (A, b, mu) on the host and the fp64 solution of (A + mu I) x = b
    for those fp32 inputs (by Cholesky above n = 1024)."""
    g = torch.Generator().manual_seed(seed)
    G = torch.randn(batch, n, n, generator=g)
    A = G @ G.transpose(1, 2) / n + 0.5 * torch.eye(n)
    b = torch.randn(batch, n, generator=g)
    mu = 0.01 + 0.99 * torch.rand(batch, generator=g)
    return A, b, mu, host_solve(A, b, mu)


def host_solve(A, b, mu):
    Ad = A.double() + mu.double()[:, None, None] * torch.eye(
        A.shape[1], dtype=torch.float64)
    if A.shape[1] <= 1024:
        return torch.linalg.solve(Ad, b.double().unsqueeze(-1)).squeeze(-1)
    return torch.cholesky_solve(b.double().unsqueeze(-1),
                                torch.linalg.cholesky(Ad)).squeeze(-1)


def direct(A, b, mu):
    ext = hip_host._ext()
    sc = torch.empty(A.shape[0], 2 * A.shape[1] ** 2, device=DEV)
    dp, info = ext.chol_solve_blocked(A.to(DEV), b.to(DEV), mu.to(DEV), sc)
    return dp.cpu(), info.cpu().tolist()


def errs(dp, ref):
    return ((dp.double() - ref).abs().max(dim=1).values
            / ref.abs().max(dim=1).values)


# one block; ragged second block (one partial strip, one partial tile); one
# full trailing tile; an off-diagonal tile with ragged trsm and update edges
@pytest.mark.parametrize('n', (X, X + 32, 2 * X, 3 * X + 64))
def test_direct_entry(n):
    A, b, mu, ref = problem(n, 3, 40 + n)
    dp, info = direct(A, b, mu)
    err = float(errs(dp, ref).max())
    print(f'n={n}: rel err {err:.3e}')
    assert info == [0, 0, 0] and err < LIM
    assert torch.equal(direct(A, b, mu)[0], dp)


@pytest.mark.parametrize('where', ('first pivot', 'second block'))
def test_failure_is_contained(where):
    n = 2 * X
    A, b, mu, _ = problem(n, 3, 51)
    if where == 'first pivot':
        A[1] = -torch.eye(n)
    else:
        A[1, X + 5, X + 5] = -10.0
    dp, info = direct(A, b, mu)
    good = [0, 2]
    assert info == [0, 1, 0] and torch.isnan(dp[1]).all()
    assert float(errs(dp[good], host_solve(A[good], b[good],
                                           mu[good])).max()) < LIM


@pytest.mark.parametrize('n', (48, 16416))
def test_refused_shapes(n):
    ext = hip_host._ext()
    A = torch.empty(1, n, n, device=DEV)
    sc = torch.empty(1, 2 * n * n, device=DEV)
    b, mu = torch.ones(1, n, device=DEV), torch.full((1,), 0.1, device=DEV)
    with pytest.raises(RuntimeError):
        ext.chol_solve_blocked(A, b, mu, sc)


def test_above_the_old_limit(monkeypatch):
    """chol_solve_damped at n = 4104 (padded to 4128), batch 2. Measured on
    an MI355X on these inputs against the fp64 host Cholesky solve: torch's
    fp32 cholesky_ex + cholesky_solve on the device, one problem at a time,
    1.15e-06; the blocked kernels 8.15e-07. Limit: 4 x torch's figure
    (capped at 5e-2, the project's limit at n = 4096), 4.6e-06. On the code
    before the blocked kernels this call fails on the n <= 4096 assertion."""
    monkeypatch.setenv('SAGECAL_CHOL_BLOCKED', '1')
    A, b, mu, ref = problem(4104, 2, 61)
    dp = hip_host.chol_solve_damped(A.to(DEV), b.to(DEV), mu.to(DEV)).cpu()
    err = float(errs(dp, ref).max())
    print(f'n=4104: rel err {err:.3e}')
    assert dp.shape == (2, 4104) and err < LIM_4104


@pytest.mark.parametrize('K', (2, 1))
def test_joint_path(monkeypatch, K):
    """lm.joint_lm_solve, 9 clusters x 57 stations x K chunks, T = 4,
    2 iterations: K = 2 is the batched loop over 2 blocks of Pb = 4104,
    K = 1 the dense loop at P = 4104; with the switch off both factor with
    torch. Measured on an MI355X at K = 2: initial cost 1.061131e+04, final
    4.290183e+00 with the switch off and 4.290182e+00 with it on, relative
    difference 2.22e-07; at K = 1: initial 1.037763e+04, final 4.732273e+00
    with either, difference 0. Limit: 10 x the larger (and no looser than
    1e-3)."""
    M, N, T = 9, 57, 4
    rng = np.random.default_rng(71)
    pairs = np.array([(p, q) for p in range(N) for q in range(p + 1, N)])
    Nbase, nchunks = len(pairs), [K] * M
    chunk_off = [ci * K for ci in range(M)]

    def cplx(*shape):
        return torch.tensor(rng.standard_normal(shape)
                            + 1j * rng.standard_normal(shape),
                            dtype=torch.complex64)
    Jt = torch.eye(2, dtype=torch.complex64) + 0.2 * cplx(M * K, N, 2, 2)
    cohs = cplx(M, T * Nbase, 2, 2)
    bb = torch.tensor(np.tile(pairs, (T, 1)))
    x = sum(R.apply_jones(cohs[ci], Jt[ci * K:(ci + 1) * K], bb,
                          R.chunk_rows_for(ci, nchunks, T, Nbase, T * Nbase,
                                           'cpu')) for ci in range(M))
    x = x + 0.01 * cplx(T * Nbase, 2, 2)
    args = (x.to(DEV), cohs.to(DEV), (Jt + 0.05 * cplx(M * K, N, 2, 2)).to(DEV),
            chunk_off, nchunks, bb.to(DEV), T, Nbase)
    init = float(ops.joint_cost(*args))
    monkeypatch.setenv('SAGECAL_JOINT_KERNEL', '1')
    _, off = lm.joint_lm_solve(*args, maxiter=2)
    monkeypatch.setenv('SAGECAL_CHOL_BLOCKED', '1')
    calls, real = [], hip_host.chol_solve_damped
    monkeypatch.setattr(hip_host, 'chol_solve_damped',
                        lambda *a: calls.append(1) or real(*a))
    _, on = lm.joint_lm_solve(*args, maxiter=2)
    assert len(calls) == 2
    print(f'initial {init:.6e} switch off {off:.6e} switch on {on:.6e} '
          f'rel diff {abs(on / off - 1):.3e}')
    assert on < init and abs(on / off - 1) < JOINT_REL
