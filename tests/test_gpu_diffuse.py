"""ops.diffuse_coherencies (k_diffuse_station and k_diffuse_pair, diffuse.hip)
on the device against shapelet.recalculate_diffuse_coherencies in complex128
on the CPU, from the same float64 draws; then the routing of
ConsensusADMM.diffuse_coherencies by SAGECAL_DIFFUSE_KERNEL and the host path
outside the kernels' range.

The error is max |V - ref| / max |ref| over the rows of live pairs, held to
1e-5, the limit tests/test_gpu_shapelet_kernel.py sets for the same float32
mode sum of k_shapelet_coh; the series products are float64 and add nothing at
that level. The rows of the flagged pair must be exactly zero. Each case
prints its figure before it asserts. Measured on an MI355X, in the order
of CASES: 2.0e-7, 2.2e-7, 3.4e-7, 3.2e-7, 3.7e-7, 1.7e-7, 2.5e-7, 5.4e-7."""
import functools
import math

import numpy as np
import pytest
import torch

from sagecal_amd import shapelet
from sagecal_amd.ops import dispatch as ops
from sagecal_amd.ops import hip_host

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FREQ, FDELTA, BETA_Z, BETA_C = 150e6, 1e6, 0.02, 0.01
LMN = (0.01, -0.02, math.sqrt(1 - 0.01 ** 2 - 0.02 ** 2) - 1)

# (N, Gz, Gc, T): the first five are the shapes of the kernels' contract
# (one mode; small; n2 = 10; n1 = 15 and n2 = 17 across the 16-wide tile;
# n2 = 32, the limit). Then n2 = 7 and n2 = 8, either side of the switch
# from plain FMA to the matrix unit, and T = 70, a second pass of the lanes
# over the timeslots.
CASES = [(3, 1, 1, 1), (5, 2, 3, 3), (6, 3, 6, 2), (4, 3, 13, 2),
         (4, 4, 26, 1), (3, 2, 5, 1), (3, 2, 6, 1), (3, 1, 2, 70)]


@functools.lru_cache(maxsize=None)
def make(N, Gz, Gc, T, seed=11):
    """Seeded inputs on the CPU and the host result: (u, v, w, pairs, Z, Cm,
    ref, live rows). |u f g2|, |v f g2| < 3; the pair table is shuffled,
    pair 0 the other way round and pair 1 flagged."""
    rng = np.random.default_rng(seed)
    cplx = lambda *s: torch.tensor(rng.standard_normal(s)
                                   + 1j * rng.standard_normal(s))
    g2 = shapelet.product_scale(
        BETA_Z, shapelet.product_scale(BETA_C, BETA_Z))
    pr = np.array([(p, q) for p in range(N) for q in range(p + 1, N)])
    pr = pr[rng.permutation(len(pr))]
    pr[0] = pr[0, ::-1]
    pr[1] = -1
    pairs = torch.tensor(pr)
    u, v, w = (torch.tensor(rng.uniform(-3, 3, T * len(pr))) / (FREQ * g2)
               for _ in range(3))
    Z, Cm = cplx(N, Gz * Gz, 2, 2), cplx(Gc * Gc, 2, 2)
    live = (pairs >= 0).all(dim=1).repeat(T)
    ref = shapelet.recalculate_diffuse_coherencies(
        u, v, w, pairs.clamp_min(0).repeat(T, 1), Z, BETA_Z, Cm, BETA_C,
        *LMN, FREQ, FDELTA)
    return u, v, w, pairs, Z, Cm, ref, live


def run_op(u, v, w, pairs, Z, Cm, T):
    return ops.diffuse_coherencies(u.to(DEV), v.to(DEV), w.to(DEV),
                                   pairs.to(DEV), T, Z, BETA_Z, Cm, BETA_C,
                                   LMN, FREQ, FDELTA)


@pytest.mark.parametrize('N,Gz,Gc,T', CASES)
def test_against_host(N, Gz, Gc, T):
    u, v, w, pairs, Z, Cm, ref, live = make(N, Gz, Gc, T)
    out = run_op(u, v, w, pairs, Z, Cm, T)
    assert out.is_cuda and out.dtype == torch.complex64
    out = out.cpu()
    err = float((out[live] - ref[live]).abs().max() / ref[live].abs().max())
    print(f'N={N} Gz={Gz} Gc={Gc} T={T}: relative error {err:.2e}')
    assert err <= 1e-5
    assert int((~live).sum()) == T and not out[~live].any()


def test_repeatable():
    u, v, w, pairs, Z, Cm, _, _ = make(*CASES[3])
    a = run_op(u, v, w, pairs, Z, Cm, CASES[3][3])
    b = run_op(u, v, w, pairs, Z, Cm, CASES[3][3])
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))


def test_routing(monkeypatch):
    from test_consensus import _band_problem
    from sagecal_amd.consensus.admm import ConsensusADMM
    from sagecal_amd.constants import SM_LM_LBFGS
    from sagecal_amd.solvers import sage
    pack, ms, tile, bb, cohs, _, freqs_all, f0 = _band_problem(0, 1)
    opts = sage.SageSolveOptions(max_emiter=2, max_iter=8,
                                 solver_mode=SM_LM_LBFGS, mode='batched')
    cent = (np.array([0.001 * i for i in range(pack.M)]),
            np.array([0.0005 * i for i in range(pack.M)]))
    adm = ConsensusADMM(sage.CalState(pack, ms.N), freqs_all, f0, 0, 1,
                        Npoly=1, rho=torch.full((pack.M,), 1.0),
                        spatial=(0.01, 1e-5, 2, 20, 1), spatial_alpha=0.0,
                        centroids=cent)
    adm.run(cohs, tile, bb, opts, n_admm=3)
    Z, bz = adm.diffuse_station_series()
    Cm = torch.zeros(4, 2, 2, dtype=torch.complex128)
    Cm[:, 0, 0] = Cm[:, 1, 1] = torch.tensor([1.0, -0.5, 0.3, 0.2])
    uvw = [t.to(DEV) for t in (tile.u, tile.v, tile.w)]
    rest = (bb, Cm, 1e-3, (1e-3, 0.0, 0.0), float(f0), 1e5)
    kw = dict(T=tile.tilesz, Nbase=tile.Nbase)
    monkeypatch.delenv('SAGECAL_DIFFUSE_KERNEL', raising=False)
    assert not ops.diffuse_kernel_on()
    host = shapelet.recalculate_diffuse_coherencies(
        tile.u.double(), tile.v.double(), tile.w.double(), bb, Z, bz, Cm,
        1e-3, 1e-3, 0.0, 0.0, float(f0), 1e5)
    off = adm.diffuse_coherencies(*uvw, *rest, **kw)
    assert not off.is_cuda and torch.equal(torch.view_as_real(off),
                                           torch.view_as_real(host))
    monkeypatch.setenv('SAGECAL_DIFFUSE_KERNEL', '1')
    assert ops.diffuse_kernel_on()
    on = adm.diffuse_coherencies(*uvw, *rest, **kw)
    op = ops.diffuse_coherencies(
        *uvw, ops.lbfgs_pair_table(bb, tile.Nbase, DEV), tile.tilesz, Z, bz,
        Cm, 1e-3, (1e-3, 0.0, 0.0), float(f0), 1e5)
    assert on.is_cuda and torch.equal(torch.view_as_real(on),
                                      torch.view_as_real(op))
    assert float((on.cpu() - host).abs().max()) <= 1e-5 * float(
        host.abs().max())
    monkeypatch.setenv('SAGECAL_FORCE_REFERENCE', '1')
    assert not ops.diffuse_kernel_on()


def test_outside_range(monkeypatch):
    """n2 = 33: the host result, and no kernel launch."""
    N, Gz, Gc, T = 3, 1, 33, 1
    u, v, w, pairs, Z, Cm, ref, live = make(N, Gz, Gc, T)
    calls = []
    monkeypatch.setattr(hip_host, 'diffuse_coherencies',
                        lambda *a, **k: calls.append(1))
    out = run_op(u, v, w, pairs, Z, Cm, T)
    assert not calls and out.is_cuda
    assert torch.equal(out.cpu()[live], ref[live]) and not out[~live].any()
