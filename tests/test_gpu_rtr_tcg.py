"""ops.rtr_tcg (k_rtr_tcg, rtr_tcg.hip) in float32 on the device against the
torch code of solvers/rtr.py (grad, _tcg_fixed, hess_vec) in float64 on the
CPU from the same inputs, and rtr_solve / rtr_solve_graphed with
SAGECAL_RTR_KERNEL=1 against the switch-off path.

The stop and boundary decisions of the CG loop are discrete, so every case
pins the number of CG iterations each chunk enters. Checked on the CPU: with
these seeds, deltas, kappas and shift the torch path enters exactly these
counts in float64 and in float32. The three deltas of a 3-chunk case are:
below the first step (boundary hit in iteration 1), 1e6 (no hit; the chunk
ends on its residual or on maxit) and between the norms after iterations
1 and 2 (or 2 and 3) of that chunk. kappa below the default 0.01 keeps the
no-hit chunk iterating where 0.01 would stop it after 3 iterations. The
shifted case makes JtJ indefinite: it ends in iteration 3 on dHd <= 0 (with
delta = 1e6 in place of 50 the count is the same, so the radius is not what
stops it).

Errors are max|a - ref| / max|ref| for g, eta, Heta and relative for the
three inner products. Largest measured on an MI355X over the cases below,
against the float64 yardstick:
  torch float32 path on the device (SAGECAL_FORCE_REFERENCE=1):
    vectors 1.62e-06 (eta, N = 64), scalars 2.76e-07
  k_rtr_tcg: vectors 8.52e-07 (eta, N = 3), scalars 2.56e-07
The limits are 4 x the torch path's figures, which allows for the kernel's
different but fixed summation order: vectors 6.5e-06, scalars 1.2e-06. Every
case entered the pinned iteration counts on both paths."""
import numpy as np
import pytest
import torch

from sagecal_amd.ops import dispatch as ops
from sagecal_amd.ops import hip_host
from sagecal_amd.ops import reference as R
from sagecal_amd.solvers import lm, rtr

gpu = pytest.mark.gpu
DEV = 'cuda:0'
VEC_LIM, SCALAR_LIM = 6.5e-6, 1.2e-6


def make_inputs(N, n, shift, seed=7):
    """(JtJ [n,8N,8N], Jtr [n,8N], J = I + 0.2 noise [n,N,2,2], iw [N]) in
    float64 / complex128: R.jtj_jtr of seeded x and coh, one timeslot of all
    N(N-1)/2 pairs per chunk, JtJ less shift * I; iw from the pair counts.
    N = 3 gets 4 timeslots: one gives 24 equations for 24 unknowns, a JtJ so
    ill-conditioned that 12 CG iterations of the torch path itself differ by
    8e-2 between float32 and float64."""
    rng = np.random.default_rng(seed)

    def cplx(*shape):
        return torch.tensor(rng.standard_normal(shape)
                            + 1j * rng.standard_normal(shape))
    pairs = np.array([(p, q) for p in range(N) for q in range(p + 1, N)])
    Nbase = len(pairs) * (4 if N == 3 else 1)
    bb = torch.tensor(np.tile(pairs, (n * Nbase // len(pairs), 1)))
    rows = torch.arange(n).repeat_interleave(Nbase)
    x, coh = cplx(n * Nbase, 2, 2), cplx(n * Nbase, 2, 2)
    J = torch.tensor(np.eye(2)[None, None]) + 0.2 * cplx(n, N, 2, 2)
    JtJ, Jtr, _ = R.jtj_jtr(x, coh, J, bb, N, None, rows, n)
    JtJ = JtJ - shift * torch.eye(8 * N, dtype=torch.float64)
    iw = torch.tensor(1.0 / np.bincount(pairs.reshape(-1), minlength=N))
    return JtJ, Jtr, J, iw


def to_dev(t):
    return t.to(DEV, torch.complex64 if t.is_complex() else torch.float32)


# N, maxit, kappa, delta per chunk, shift, CG iterations entered per chunk
CASES = [
    (3, 12, 1e-4, (0.5, 1e6, 2.0), 0.0, (1, 11, 2)),    # P = 24 < a wave
    (8, 12, 1e-4, (0.5, 1e6, 3.27), 0.0, (1, 12, 2)),   # P = 64
    (9, 12, 1e-4, (0.5, 1e6, 3.9), 0.0, (1, 11, 3)),    # P = 72
    (33, 12, 1e-6, (0.5, 1e6, 6.21), 0.0, (1, 10, 2)),  # P = 264
    (64, 12, 1e-6, (0.5, 1e6, 8.75), 0.0, (1, 9, 2)),   # P = 512
    (3, 1, 1e-2, (1e6,), 0.0, (1,)),
    (33, 1, 1e-2, (1e6,), 0.0, (1,)),
    (64, 12, 1e-2, (1e6,), 0.0, (3,)),                  # the defaults
    (9, 12, 1e-2, (50.0,), 19.4, (3,)),                 # indefinite
]


@gpu
@pytest.mark.parametrize('N,maxit,kappa,delta,shift,nit', CASES)
def test_against_float64(N, maxit, kappa, delta, shift, nit):
    inp = make_inputs(N, len(delta), shift)
    delta = torch.tensor(delta, dtype=torch.float64)
    *ref, st_ref = ops.rtr_tcg(*inp, delta, maxit, kappa)
    assert st_ref[:, 3].tolist() == list(nit)
    dev = [to_dev(t) for t in (*inp, delta)]
    *out, st = ops.rtr_tcg(*dev, maxit, kappa)
    ev = [float((a.cpu().to(b.dtype) - b).abs().max() / b.abs().max())
          for a, b in zip(out, ref)]
    es = float((st[:, :3].cpu().double() / st_ref[:, :3] - 1).abs().max())
    print(f'N={N} maxit={maxit} shift={shift}: g {ev[0]:.2e} eta {ev[1]:.2e} '
          f'Heta {ev[2]:.2e} scalars {es:.2e} nit {st[:, 3].tolist()}')
    assert st[:, 3].tolist() == list(nit)
    assert max(ev) < VEC_LIM and es < SCALAR_LIM
    again = ops.rtr_tcg(*dev, maxit, kappa)
    assert all(torch.equal(a, b) for a, b in zip((*out, st), again))


@gpu
@pytest.mark.parametrize('solve', ('rtr_solve', 'rtr_solve_graphed'))
def test_solver_switch(monkeypatch, solve):
    """N = 5, T = 4, two chunks, noiseless data of a known J, from identity,
    20 outer iterations. Measured on an MI355X, the same for both solvers:
    initial cost 3.9979e+01, final 6.3368e-13 with the switch off and
    6.9314e-13 with it on."""
    N, T, n = 5, 4, 2
    rng = np.random.default_rng(11)
    pairs = np.array([(p, q) for p in range(N) for q in range(p + 1, N)])
    Nbase = len(pairs)
    bb = torch.tensor(np.tile(pairs, (T, 1)))
    rows = (torch.arange(T) // (T // n)).repeat_interleave(Nbase)
    s = torch.tensor(rng.standard_normal(T * Nbase)
                     + 1j * rng.standard_normal(T * Nbase))
    coh = s[:, None, None] * torch.eye(2, dtype=torch.complex128)
    Jt = torch.tensor(np.eye(2)[None, None] + 0.2 * (
        rng.standard_normal((n, N, 2, 2))
        + 1j * rng.standard_normal((n, N, 2, 2))))
    x = R.apply_jones(coh, Jt, bb, rows)
    bb, rows = bb.to(DEV), rows.to(DEV)
    prob = lm.LMProblem(
        x.to(DEV, torch.complex64), coh.to(DEV, torch.complex64), bb, N, n,
        rows, layout=hip_host.BaselineLayout(bb, Nbase, T, 1, N, DEV))
    J0 = torch.eye(2, dtype=torch.complex64, device=DEV).expand(
        n, N, 2, 2).contiguous()
    monkeypatch.setenv('SAGECAL_RTR_GRAPH', '0')    # rtr_solve stays eager
    _, off = getattr(rtr, solve)(prob, J0, maxiter=20)
    calls = []
    real = hip_host.rtr_tcg
    monkeypatch.setattr(hip_host, 'rtr_tcg',
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setenv('SAGECAL_RTR_KERNEL', '1')
    _, on = getattr(rtr, solve)(prob, J0, maxiter=20)
    init = float(on['init_cost'].sum())
    off, on = float(off['final_cost'].sum()), float(on['final_cost'].sum())
    print(f'{solve}: initial {init:.4e} switch off {off:.4e} '
          f'switch on {on:.4e}')
    assert len(calls) > 0
    assert on <= 2 * off and on < 1e-6 * init


def test_cpu_wraps_the_torch_code():
    JtJ, Jtr, J, iw = make_inputs(5, 2, 0.0)
    delta = torch.tensor([0.5, 1e6], dtype=torch.float64)
    g, eta, Heta, st = ops.rtr_tcg(JtJ, Jtr, J, iw, delta, maxit=4)
    obj = rtr._Objective(None, iw)
    obj.JtJ, obj.Jtr = JtJ, Jtr
    g_ref = obj.grad(J)
    eta_ref = rtr._tcg_fixed(obj, J, g_ref, delta, 4)
    He_ref = obj.hess_vec(J, eta_ref)
    assert torch.equal(g, g_ref) and torch.equal(eta, eta_ref)
    assert torch.equal(Heta, He_ref)
    assert torch.equal(st[:, :3], torch.stack(
        [rtr._inner(g_ref, g_ref), rtr._inner(g_ref, eta_ref),
         rtr._inner(eta_ref, He_ref)], -1))
    assert st[:, 3].tolist() == [1.0, 4.0]
