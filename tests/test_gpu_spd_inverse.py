"""ops.spd_inverse_damped (spd_inverse.hip) on the device against
torch.linalg.inv(A.double() + mu I) on the CPU, for A = sym(G G^T / 2n) in
float32 from G = standard_normal((b, n, 2n)), seed n, and mu = 1e-2.

Limit per matrix: max |X - X_ref| <= 8 n eps cond2(A + mu I) ||X_ref||_2 with
eps = 2^-52, the forward bound of a Cholesky-based inverse, computed from the
reference. On the CPU cond2 is 14 to 46 for these shapes, the limit 1e-12 to
6e-10 against max |X| of 2 to 5, and two correct float64 inverses differ by
7e-6 to 1.4e-3 of it; a float32 intermediate (1e-7) is far outside. The block
edges of the kernels are the multiples of 32: 8 and 24 stay inside one block,
40, 136 and 520 end in a ragged one.

Measured on an MI355X, max |X - X_ref| / limit over the matrices of a case:
(8, 1) 6.9e-4, (24, 300) 6.0e-4, (40, 3) 1.9e-4, (136, 3) 7.6e-5, (512, 2)
3.1e-5, (520, 1) 3.3e-5, (1024, 1) 2.4e-5, the same for float64 A, (40, 3)
with per-matrix mu 3.4e-3; max |X - X_ref| 6.7e-16 to 1.4e-14.

test_through_diagnostics_leverage (N = 8, T = 4, 2 chunks, mu = 1e-6, max
lev 2.88): the float32 JtJ that the device assembles for chunk 0 has the
eigenvalue -1.45e-6 along its gauge direction (0 in exact arithmetic, -5.5e-14
in the float64 assembly), so JtJ + 1e-6 I is not positive definite,
torch.linalg.cholesky_ex on the CPU stops at pivot 64 on the same matrix, and
the kernels flag it and return NaN as their contract says. The diagnostic
inverts such a chunk by torch.linalg.inv, as it does without the switch, and
chunk 1 comes from the kernels. Measured on an MI355X against the complex128
CPU result: with the switch 1.28e-07, without 1.25e-07. At mu = 1e-5, 1e-4
and 1e-2, where both chunks are positive definite and go through the kernels,
the two paths' errors are 1.2372e-07 against 1.2389e-07, 1.23360e-07 against
1.23363e-07 and 1.232843e-07 against 1.232841e-07."""
import functools

import numpy as np
import pytest
import torch

from sagecal_amd.ops import dispatch as ops
from sagecal_amd.ops import hip_host
from sagecal_amd.ops import reference as R
from sagecal_amd.solvers import diagnostics as diag
from test_gpu_leverage import solve_inputs

gpu = pytest.mark.gpu
DEV = 'cuda:0'
MU = (1e-2,)
MU3 = (1e-2, 1.0, 1e-1)
F32, F64 = torch.float32, torch.float64


@functools.lru_cache(maxsize=None)
def make(n, b, mus=MU):
    """Seeded A [b, n, n] float32 on the CPU, inv(A + mu I) in float64, and
    per matrix cond2(A + mu I) and the limit."""
    rng = np.random.default_rng(n)
    G = torch.tensor(rng.standard_normal((b, n, 2 * n)).astype(np.float32))
    A = G @ G.mT / (2 * n)
    A = (A + A.mT) / 2
    Ad = A.double() + torch.tensor(mus, dtype=F64).reshape(-1, 1, 1) \
        * torch.eye(n, dtype=F64)
    ref = torch.linalg.inv(Ad)
    sv = torch.linalg.svdvals(Ad)
    cond = sv[:, 0] / sv[:, -1]
    limit = 8 * n * 2.0 ** -52 * cond * torch.linalg.svdvals(ref)[:, 0]
    return A, ref, cond, limit


def mu_arg(mus):
    return mus[0] if len(mus) == 1 else torch.tensor(mus, dtype=F64)


@gpu
@pytest.mark.parametrize('n,b,dtype,mus', [
    (8, 1, F32, MU), (24, 300, F32, MU), (40, 3, F32, MU), (136, 3, F32, MU),
    (512, 2, F32, MU), (520, 1, F32, MU), (1024, 1, F32, MU),
    (40, 3, F64, MU), (136, 3, F64, MU), (40, 3, F32, MU3)])
def test_against_linalg_inv(n, b, dtype, mus):
    A, ref, cond, limit = make(n, b, mus)
    assert float(cond.max()) <= 1e3, cond
    Ad = A.to(DEV, dtype)
    X = ops.spd_inverse_damped(Ad, mu_arg(mus))
    assert X.dtype == F64 and X.shape == ref.shape
    assert torch.equal(X, X.mT)
    assert torch.equal(X, ops.spd_inverse_damped(Ad, mu_arg(mus)))
    assert torch.equal(Ad.cpu(), A.to(dtype))            # input untouched
    err = (X.cpu() - ref).abs().amax(dim=(1, 2))
    print(f'n {n} b {b} {dtype} mu {mus}: cond {float(cond.max()):.1f} '
          f'max|X| {float(ref.abs().max()):.2f} err {float(err.max()):.2e} '
          f'limit {float(limit.min()):.2e} err/limit '
          f'{float((err / limit).max()):.2e}')
    assert bool((err <= limit).all())


@gpu
def test_batch_independence():
    A = make(136, 3)[0].to(DEV)
    assert torch.equal(ops.spd_inverse_damped(A, MU[0])[1],
                       ops.spd_inverse_damped(A[1:2].clone(), MU[0])[0])


@gpu
def test_failure_flag():
    A = make(40, 3)[0].to(DEV)
    clean = ops.spd_inverse_damped(A, MU[0])
    B = A.clone()
    B[1] = -torch.eye(40, device=DEV)
    X, info = hip_host.spd_inverse_damped(B, MU[0], return_info=True)
    assert bool(X[1].isnan().all())
    assert [bool(i) for i in info.cpu()] == [False, True, False]
    assert torch.equal(X[0], clean[0]) and torch.equal(X[2], clean[2])


def test_cpu_path(monkeypatch):
    """Off the device: the torch formula, whole and in pieces."""
    A = make(24, 300)[0][:5]
    eye = torch.eye(24, dtype=F64)
    old = torch.linalg.inv(A.to(F64) + MU[0] * eye)
    assert torch.equal(ops.spd_inverse_damped(A, MU[0]), old)
    monkeypatch.setattr(ops, 'INVERSE_SPLIT_ENTRIES', 2 * 24 * 24)
    pieces = torch.cat([torch.linalg.inv(A[i:i + 2].to(F64) + MU[0] * eye)
                        for i in (0, 2, 4)])
    assert torch.equal(ops.spd_inverse_damped(A, MU[0]), pieces)
    assert not ops.inverse_kernel_on()
    monkeypatch.setenv('SAGECAL_INVERSE_KERNEL', '1')
    assert ops.inverse_kernel_on()
    monkeypatch.setenv('SAGECAL_FORCE_REFERENCE', '1')
    assert not ops.inverse_kernel_on()


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
    real = hip_host.spd_inverse_damped
    monkeypatch.setattr(hip_host, 'spd_inverse_damped',
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.delenv('SAGECAL_INVERSE_KERNEL', raising=False)
    off = diag.leverage(*args, **kw).cpu()
    assert len(calls) == 0
    monkeypatch.setenv('SAGECAL_INVERSE_KERNEL', '1')
    on = diag.leverage(*args, **kw).cpu()
    assert len(calls) == 1
    e_on = float((on - ref).abs().max())
    e_off = float((off - ref).abs().max())
    print(f'max lev {float(ref.max()):.3f}: inverse kernels {e_on:.2e}, '
          f'torch.linalg.inv {e_off:.2e}')
    assert e_on <= 4 * e_off
