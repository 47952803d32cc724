"""GPU numerics tests: HIP kernels vs the fp32/fp64 PyTorch reference.

Every test is marked gpu and compares the gfx950 kernel output against the
same op computed by the plain PyTorch reference implementation (fp64 on
CPU), with fp32-appropriate tolerances.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def problem():
    from sagecal_amd import sky, msdata
    from sagecal_amd.ops.reference import SourcePack
    srcs, clist = sky.make_synthetic_sky(M=3, nsrc_per_cluster=4, seed=5)
    # make one cluster extended: gaussian + disk + ring
    names = list(srcs)
    srcs[names[0]].stype = 1
    srcs[names[0]].eX = srcs[names[0]].eY = 0.001
    srcs[names[0]].eP = 0.4
    srcs[names[1]].stype = 2
    srcs[names[1]].eX = srcs[names[1]].eY = 0.0007
    srcs[names[2]].stype = 3
    srcs[names[2]].eX = srcs[names[2]].eY = 0.0005
    clusters = sky.build_clusters(srcs, clist, 0.0, np.pi / 4, 150e6)
    pack = SourcePack(clusters)
    ms = msdata.SyntheticMS(N=14, tilesz=6, Ntime=6, Nchan=2, pack=pack,
                            bandwidth=120e3, noise_sigma=1e-3, seed=7)
    tile = ms.load_tile(0)
    bb = ms.bb_tensor()
    return pack, ms, tile, bb


def test_ext_loads():
    from sagecal_amd.ops import dispatch
    assert dispatch.have_ext(), f"extension failed: {dispatch._ext_err}"


def test_predict_coh_matches_reference(problem):
    from sagecal_amd.ops import reference as R
    from sagecal_amd.ops import hip_host
    pack, ms, tile, bb = problem
    ref = R.predict_coh(pack, tile.u, tile.v, tile.w, tile.freq0,
                        tile.freq0, tile.fdelta, tile.tdelta, tile.dec0)
    dev = 'cuda:0'
    got = hip_host.predict_coh(pack, tile.u.to(dev), tile.v.to(dev),
                               tile.w.to(dev), tile.freq0, tile.freq0,
                               tile.fdelta, tile.tdelta, tile.dec0)
    got = got.cpu().to(torch.complex128)
    scale = float(ref.abs().max())
    err = (got - ref).abs().max() / scale
    assert float(err) < 5e-6, f"predict mismatch: rel err {float(err)}"


def test_jtj_jtr_matches_reference(problem):
    from sagecal_amd.ops import reference as R
    from sagecal_amd.ops.hip_host import BaselineLayout, jtj_jtr
    pack, ms, tile, bb = problem
    N = ms.N
    rng = np.random.default_rng(3)
    cohs = R.predict_coh(pack, tile.u, tile.v, tile.w, tile.freq0,
                         tile.freq0, tile.fdelta, tile.tdelta, tile.dec0)
    J = torch.tensor(np.eye(2)[None, None]
                     + 0.2 * (rng.standard_normal((1, N, 2, 2))
                              + 1j * rng.standard_normal((1, N, 2, 2))))
    w = torch.tensor(rng.uniform(0.5, 2.0, tile.x.shape[0]))
    JtJ_r, Jtr_r, cost_r = R.jtj_jtr(tile.x, cohs[0], J, bb, N, w, None, 1)
    dev = 'cuda:0'
    lay = BaselineLayout(bb.to(dev), ms.Nbase, tile.tilesz, 1, N, dev)
    JtJ_g, Jtr_g, cost_g = jtj_jtr(
        tile.x.to(device=dev, dtype=torch.complex64),
        cohs[0].to(device=dev, dtype=torch.complex64),
        J.to(device=dev, dtype=torch.complex64), bb.to(dev), N,
        w.to(device=dev, dtype=torch.float32), None, 1, lay)
    sc = float(JtJ_r.abs().max())
    err = (JtJ_g.cpu().double() - JtJ_r).abs().max() / sc
    assert float(err) < 2e-5, f"JtJ mismatch {float(err)}"
    scg = float(Jtr_r.abs().max())
    errg = (Jtr_g.cpu().double() - Jtr_r).abs().max() / scg
    assert float(errg) < 2e-5, f"Jtr mismatch {float(errg)}"
    assert float(cost_g) == pytest.approx(float(cost_r), rel=1e-4)


def test_jtj_jtr_chunked(problem):
    from sagecal_amd.ops import reference as R
    from sagecal_amd.ops.hip_host import BaselineLayout, jtj_jtr
    pack, ms, tile, bb = problem
    N = ms.N
    B = tile.x.shape[0]
    rng = np.random.default_rng(4)
    cohs = R.predict_coh(pack, tile.u, tile.v, tile.w, tile.freq0,
                         tile.freq0, tile.fdelta, tile.tdelta, tile.dec0)
    nchunk = 3
    rows = R.chunk_rows_for(0, [nchunk], tile.tilesz, ms.Nbase, B, 'cpu')
    J = torch.tensor(np.eye(2)[None, None]
                     + 0.2 * (rng.standard_normal((nchunk, N, 2, 2))
                              + 1j * rng.standard_normal((nchunk, N, 2, 2))))
    JtJ_r, Jtr_r, _ = R.jtj_jtr(tile.x, cohs[0], J, bb, N, None, rows,
                                nchunk)
    dev = 'cuda:0'
    lay = BaselineLayout(bb.to(dev), ms.Nbase, tile.tilesz, 1, N, dev)
    JtJ_g, Jtr_g, _ = jtj_jtr(
        tile.x.to(device=dev, dtype=torch.complex64),
        cohs[0].to(device=dev, dtype=torch.complex64),
        J.to(device=dev, dtype=torch.complex64), bb.to(dev), N,
        None, rows.to(dev), nchunk, lay)
    sc = float(JtJ_r.abs().max())
    err = (JtJ_g.cpu().double() - JtJ_r).abs().max() / sc
    assert float(err) < 2e-5
    errg = (Jtr_g.cpu().double() - Jtr_r).abs().max() / float(Jtr_r.abs().max())
    assert float(errg) < 2e-5


def test_jtj_cost_segments_reproducible():
    """Store-and-sum accumulation at a shape the small fixture does not
    reach: N=70 (> one 64-lane pass over partner stations, not a multiple),
    two segments with two uneven time chunks each, weights, and two
    flagged baselines whose slots are never written (the scratch is
    poisoned with NaN first, and the cached pair-index table still lists
    them, so both skip paths run). JtJ, Jtr and the PER-CHUNK costs of
    both kernels match the fp64 reference, and a second call returns
    bitwise the same (no arrival-order sums). A gradient-only launch over
    segment 0 alone must fill chunks 0-1 and leave chunks 2-3 zero."""
    from sagecal_amd.ops import reference as R
    from sagecal_amd.ops.hip_host import (BaselineLayout, jtj_jtr,
                                          model_cost_per_chunk, _ext, _c64)
    dev = 'cuda:0'
    rng = np.random.default_rng(12)
    N, T, nseg, nchunk = 70, 5, 2, 4
    pairs = np.array([(p, q) for p in range(N) for q in range(p + 1, N)])
    Nbase = len(pairs)
    B = nseg * T * Nbase
    bb = torch.tensor(np.tile(pairs, (nseg * T, 1)))
    slot = np.arange(nseg * T)
    rows = torch.tensor(np.repeat(2 * (slot // T) + (slot % T >= 3), Nbase))

    def cplx(*shape):
        return torch.tensor(rng.standard_normal(shape)
                            + 1j * rng.standard_normal(shape))
    x, coh = cplx(B, 2, 2), cplx(B, 2, 2)
    J = torch.tensor(np.eye(2)[None, None]) + 0.2 * cplx(nchunk, N, 2, 2)
    w = torch.tensor(rng.uniform(0.5, 2.0, B))
    flagged = (7, 2000)                  # pair indices; reference: weight 0
    bbf = bb.clone()
    for k in flagged:
        w[k::Nbase] = 0.0
        bbf[k::Nbase] = -1
    JtJ_r, Jtr_r, _ = R.jtj_jtr(x, coh, J, bb, N, w, rows, nchunk)
    r = x - R.apply_jones(coh, J, bb, rows)
    e2 = w * (r.abs() ** 2).sum(dim=(-1, -2))
    cost_r = torch.zeros(nchunk, dtype=torch.float64).index_add_(0, rows, e2)

    BaselineLayout(bb.to(dev), Nbase, T, nseg, N, dev)   # caches full pidx
    lay = BaselineLayout(bbf.to(dev), Nbase, T, nseg, N, dev)
    assert int(lay.pidx[0, 8]) == 7 and int(lay.pairs[7, 0]) == -1
    xg = x.to(device=dev, dtype=torch.complex64)
    cg = coh.to(device=dev, dtype=torch.complex64)
    Jg = J.to(device=dev, dtype=torch.complex64)
    wg = torch.tensor(rng.uniform(0.5, 2.0, B)).to(
        device=dev, dtype=torch.float32)     # nonzero on flagged rows too
    keep = torch.ones(B, dtype=torch.bool)
    for k in flagged:
        keep[k::Nbase] = False
    wg[keep.to(dev)] = w[keep].to(device=dev, dtype=torch.float32)
    rg = rows.to(dev)

    def poison():
        # freed NaN blocks of the scratch sizes: the caching allocator
        # hands them to the next torch::empty of that size
        for shape, dt in (((nchunk * Nbase, 8), torch.complex64),
                          ((nchunk * Nbase, 8), torch.complex64),
                          ((nchunk * Nbase,), torch.float32)):
            torch.full(shape, float('nan'), dtype=dt, device=dev)
    outs = []
    for _ in range(2):
        poison()
        JtJ_g, Jtr_g, cost_g = _ext().jtj_jtr(
            _c64(xg), _c64(cg), Jg.reshape(-1, 4).contiguous(), lay.pairs,
            lay.chunk_tab(rg), lay.pidx, wg, Nbase, T, N, nseg, nchunk)
        mc_g = model_cost_per_chunk(xg, cg, Jg, bb.to(dev), N, wg, rg,
                                    nchunk, lay)
        outs.append((JtJ_g, Jtr_g, cost_g, mc_g))
    for a, b2 in zip(*outs):
        assert torch.equal(a, b2)
    JtJ_g, Jtr_g, cost_g, mc_g = outs[0]
    # fp32 sums of up to 3*2415 O(10) terms against fp64: ~1e-6 relative
    err = (JtJ_g.cpu().double() - JtJ_r).abs().max() / JtJ_r.abs().max()
    assert float(err) < 2e-5, float(err)
    errg = (Jtr_g.cpu().double() - Jtr_r).abs().max() / Jtr_r.abs().max()
    assert float(errg) < 2e-5, float(errg)
    assert torch.allclose(cost_g.cpu().double(), cost_r, rtol=1e-5)
    assert torch.allclose(mc_g.cpu().double(), cost_r, rtol=1e-5)

    # gradient-only launch that covers a subset of the chunks: segment 0
    # (chunks 0, 1) of Mt=4
    B0 = T * Nbase
    lay0 = BaselineLayout(bbf[:B0].to(dev), Nbase, T, 1, N, dev)
    poison()
    g, _ = _ext().jtr_grad(
        _c64(xg[:B0]), _c64(cg[:B0]), Jg.reshape(-1, 4).contiguous(),
        lay0.pairs, lay0.chunk_tab(rg[:B0]), lay0.pidx, wg[:B0].contiguous(),
        Nbase, T, N, 1, nchunk)
    gv = torch.view_as_real(g).reshape(nchunk, 8 * N).cpu().double()
    assert torch.isfinite(gv).all()
    assert float(gv[2:].abs().max()) == 0.0
    errs = (gv[:2] - Jtr_r[:2]).abs().max() / Jtr_r[:2].abs().max()
    assert float(errs) < 2e-5, float(errs)


def test_apply_jones_and_cost(problem):
    from sagecal_amd.ops import reference as R
    from sagecal_amd.ops.hip_host import (BaselineLayout, apply_jones,
                                          model_cost_per_chunk)
    pack, ms, tile, bb = problem
    N = ms.N
    rng = np.random.default_rng(5)
    cohs = R.predict_coh(pack, tile.u, tile.v, tile.w, tile.freq0,
                         tile.freq0, tile.fdelta, tile.tdelta, tile.dec0)
    J = torch.tensor(np.eye(2)[None, None]
                     + 0.2 * (rng.standard_normal((1, N, 2, 2))
                              + 1j * rng.standard_normal((1, N, 2, 2))))
    V_r = R.apply_jones(cohs[0], J, bb)
    dev = 'cuda:0'
    lay = BaselineLayout(bb.to(dev), ms.Nbase, tile.tilesz, 1, N, dev)
    V_g = apply_jones(cohs[0].to(device=dev, dtype=torch.complex64),
                      J.to(device=dev, dtype=torch.complex64),
                      bb.to(dev), None, lay)
    err = (V_g.cpu().to(torch.complex128) - V_r).abs().max() / float(V_r.abs().max())
    assert float(err) < 5e-6
    cost_r = float(((tile.x - V_r).abs() ** 2).sum())
    cost_g = model_cost_per_chunk(
        tile.x.to(device=dev, dtype=torch.complex64),
        cohs[0].to(device=dev, dtype=torch.complex64),
        J.to(device=dev, dtype=torch.complex64), bb.to(dev), N,
        None, None, 1, lay)
    assert float(cost_g.sum()) == pytest.approx(cost_r, rel=1e-4)


def test_gpu_sagefit_end_to_end(problem):
    """Full SAGE calibration on GPU through the HIP kernels converges."""
    from sagecal_amd.solvers import sage
    from sagecal_amd.constants import SM_RLM_RLBFGS
    pack, ms, tile, bb = problem
    dev = 'cuda:0'
    class T2:  # shallow device copy of the tile
        pass
    t2 = T2()
    for k in ('freqs', 'freq0', 'fdelta', 'tdelta', 'tilesz', 'Nbase',
              'dec0'):
        setattr(t2, k, getattr(tile, k))
    t2.u = tile.u.to(dev); t2.v = tile.v.to(dev); t2.w = tile.w.to(dev)
    t2.x = tile.x.to(device=dev, dtype=torch.complex64)
    t2.xo = tile.xo.to(device=dev, dtype=torch.complex64)
    t2.flags = tile.flags.to(dev)
    bbd = bb.to(dev)
    state = sage.CalState(pack, ms.N, device=dev, dtype=torch.complex64)
    cohs = sage.precalc_coherencies(pack, t2).to(torch.complex64)
    opts = sage.SageSolveOptions(max_emiter=3, max_iter=10,
                                 solver_mode=SM_RLM_RLBFGS, robust_outer=2)
    res0, res1 = sage.sagefit(state, cohs, t2, bbd, opts)
    assert res1 < 0.2 * res0, f"GPU sagefit: {res0} -> {res1}"


def test_chol_solve_kernel():
    """Fused damped-Cholesky kernel vs torch.linalg solve."""
    from sagecal_amd.ops.hip_host import chol_solve_damped
    dev = 'cuda:0'
    rng = np.random.default_rng(11)
    for n, batch in ((512, 3), (112, 2), (96, 1)):
        Araw = torch.tensor(rng.standard_normal((batch, n, n)),
                            dtype=torch.float32)
        A = (Araw @ Araw.transpose(-1, -2)) / n + \
            0.1 * torch.eye(n).unsqueeze(0)
        b = torch.tensor(rng.standard_normal((batch, n)),
                         dtype=torch.float32)
        mu = torch.tensor(rng.uniform(0.01, 1.0, batch),
                          dtype=torch.float32)
        ref = torch.linalg.solve(
            A.double() + mu.double()[:, None, None] * torch.eye(n).double(),
            b.double().unsqueeze(-1)).squeeze(-1)
        dp = chol_solve_damped(A.to(dev), b.to(dev), mu.to(dev))
        err = (dp.cpu().double() - ref).abs().max() / ref.abs().max()
        assert float(err) < 1e-3, f"n={n} batch={batch}: rel err {float(err)}"


def test_predict_shapelet_matches_reference():
    """HIP predict path with a shapelet cluster (kernel handles the
    non-shapelet sources; host torch adds the shapelet term) matches the
    fp64 torch reference."""
    from sagecal_amd import sky, shapelet, msdata
    from sagecal_amd.ops.reference import SourcePack
    from sagecal_amd.ops import reference as R
    from sagecal_amd.ops import hip_host
    srcs, clist = sky.make_synthetic_sky(M=2, nsrc_per_cluster=3, seed=9)
    name = clist[0][2][0]
    s = srcs[name]
    s.stype = 4
    s.eX = s.eY = 1.0
    s.sh_n0 = 3
    s.sh_beta = 1e-3
    s.sh_coeff = np.array([1.0, 0.3, 0.1, 0.2, 0.05, 0.01, 0.1, 0.02,
                           0.005])
    clusters = sky.build_clusters(srcs, clist, 0.0, np.pi / 4, 150e6)
    pack = SourcePack(clusters)
    assert pack.shapelets
    ms = msdata.SyntheticMS(N=10, tilesz=4, Ntime=4, Nchan=1, pack=None,
                            seed=13)
    tile = ms.load_tile(0)
    ref = R.predict_coh(pack, tile.u, tile.v, tile.w, 150e6, 150e6,
                        30e3, 5.0, np.pi / 4)
    dev = 'cuda:0'
    got = hip_host.predict_coh(pack, tile.u.to(dev), tile.v.to(dev),
                               tile.w.to(dev), 150e6, 150e6, 30e3, 5.0,
                               np.pi / 4)
    err = (got.cpu().to(torch.complex128) - ref).abs().max() / \
        ref.abs().max()
    assert float(err) < 1e-5, float(err)


def test_lbfgs_cost_grad_gpu():
    """GPU grad-only kernel path vs the fp64 torch reference."""
    from sagecal_amd.ops import reference as R
    from sagecal_amd.ops import hip_host
    rng = np.random.default_rng(21)
    N, T = 10, 4
    pairs = [(p, q) for p in range(N) for q in range(p + 1, N)]
    Nbase = len(pairs)
    B = Nbase * T
    bb = torch.tensor(pairs * T)
    cohs = torch.tensor(rng.standard_normal((2, B, 2, 2))
                        + 1j * rng.standard_normal((2, B, 2, 2)))
    J = torch.tensor(np.eye(2)[None, None]
                     + 0.2 * (rng.standard_normal((3, N, 2, 2))
                              + 1j * rng.standard_normal((3, N, 2, 2))))
    x = torch.tensor(rng.standard_normal((B, 2, 2))
                     + 1j * rng.standard_normal((B, 2, 2)))
    chunk_off = [0, 1]
    nchunks = [1, 2]
    for nu in (None, 5.0):
        c_ref, g_ref = R.lbfgs_cost_grad(x, cohs, J, chunk_off, nchunks,
                                         bb, T, Nbase, robust_nu=nu)
        dev = 'cuda:0'
        c_g, g_g = hip_host.lbfgs_cost_grad(
            x.to(device=dev, dtype=torch.complex64),
            cohs.to(device=dev, dtype=torch.complex64),
            J.to(device=dev, dtype=torch.complex64), chunk_off, nchunks,
            bb.to(dev), T, Nbase, robust_nu=nu)
        assert float(c_g) == pytest.approx(float(c_ref), rel=2e-4)
        err = (g_g.cpu().double() - g_ref).abs().max() / \
            float(g_ref.abs().max())
        assert float(err) < 1e-4, float(err)


def test_chol_mw_matches_single_kernel():
    """Multi-workgroup right-looking path vs the fused single-WG kernel
    (same scratch contract; dispatch picks mw for n >= 384)."""
    import sagecal_amd.ops.hip.dirac_hip as ext
    dev = 'cuda:0'
    rng = np.random.default_rng(5)
    n, batch = 512, 4
    Araw = torch.tensor(rng.standard_normal((batch, n, n)),
                        dtype=torch.float32, device=dev)
    A = ((Araw @ Araw.transpose(-1, -2)) / n
         + 0.5 * torch.eye(n, device=dev).unsqueeze(0)).contiguous()
    b = torch.tensor(rng.standard_normal((batch, n)), dtype=torch.float32,
                     device=dev).contiguous()
    mu = torch.full((batch,), 0.1, device=dev)
    sc = torch.empty(batch, 2 * n * n, dtype=torch.float32, device=dev)
    x1, i1 = ext.chol_solve(A, b, mu, sc)
    x2, i2 = ext.chol_solve_mw(A, b, mu, sc)
    assert int(i1.sum()) == 0 and int(i2.sum()) == 0
    err = (x1 - x2).abs().max() / x1.abs().max()
    assert float(err) < 1e-4, f"mw vs single rel err {float(err)}"


def _chol_problem(rng, n, batch):
    """fp32 (A, b, mu) with A = G G^T / n + 0.5 I, and the fp64 host
    solution of (A + mu I) x = b for those fp32 inputs."""
    G = rng.standard_normal((batch, n, n))
    A = torch.tensor(G @ G.transpose(0, 2, 1) / n + 0.5 * np.eye(n),
                     dtype=torch.float32)
    b = torch.tensor(rng.standard_normal((batch, n)), dtype=torch.float32)
    mu = torch.tensor(rng.uniform(0.01, 1.0, batch), dtype=torch.float32)
    ref = torch.linalg.solve(
        A.double() + mu.double()[:, None, None] * torch.eye(n).double(),
        b.double().unsqueeze(-1)).squeeze(-1)
    return A, b, mu, ref


def _chol_direct(entry, A, b, mu, dev='cuda:0'):
    batch, n = b.shape
    sc = torch.empty(batch, 2 * n * n, dtype=torch.float32, device=dev)
    dp, info = entry(A.to(dev), b.to(dev), mu.to(dev), sc)
    return dp.cpu().double(), info.cpu()


def test_chol_small_and_chunked_shapes():
    """Both Cholesky entry points, called directly, vs an fp64 host solve:
    n=32 is a single panel (the left-looking update never runs), n=64 has
    one update and one SYRK tile, n=96 three SYRK tiles (one off-diagonal:
    the tile-index decode), and n=1088 takes the chunked panel kernel with
    two panels of 1024+64 and 1024+32 rows before the single-pass ones.
    Shapes outside the kernels' contract are refused before any launch."""
    import sagecal_amd.ops.hip.dirac_hip as ext
    rng = np.random.default_rng(31)
    fused, mw = ext.chol_solve, ext.chol_solve_mw
    for n, batch, entries in ((32, 3, (fused,)), (64, 3, (fused, mw)),
                              (96, 3, (fused, mw)), (1088, 2, (mw,))):
        A, b, mu, ref = _chol_problem(rng, n, batch)
        for entry in entries:
            dp, info = _chol_direct(entry, A, b, mu)
            err = float((dp - ref).abs().max() / ref.abs().max())
            name = 'mw' if entry is mw else 'fused'
            print(f"{name} n={n} batch={batch}: rel err {err:.3e}")
            assert info.tolist() == [0] * batch, (name, n, info.tolist())
            assert err < 1e-3, f"{name} n={n} batch={batch}: rel err {err}"
    # n not a multiple of 32, and n above the fused kernel's 1024
    for n in (48, 1056):
        A = torch.eye(n).unsqueeze(0)
        with pytest.raises(RuntimeError):
            _chol_direct(fused, A, torch.ones(1, n), torch.full((1,), 0.1))


def test_chol_failed_factorization_is_contained():
    """A problem whose first pivot is negative (-I with mu = 0.1) comes
    back as a NaN row with info = 1; its neighbours in the batch are
    solved as usual."""
    import sagecal_amd.ops.hip.dirac_hip as ext
    n, batch = 64, 3
    A, b, _, _ = _chol_problem(np.random.default_rng(32), n, batch)
    A[1] = -torch.eye(n)
    mu = torch.full((batch,), 0.1)
    good = [0, 2]
    ref = torch.linalg.solve(
        A[good].double() + float(mu[0]) * torch.eye(n).double(),
        b[good].double().unsqueeze(-1)).squeeze(-1)
    for entry in (ext.chol_solve, ext.chol_solve_mw):
        dp, info = _chol_direct(entry, A, b, mu)
        assert info.tolist() == [0, 1, 0]
        assert torch.isnan(dp[1]).all()
        err = (dp[good] - ref).abs().max(dim=1).values / \
            ref.abs().max(dim=1).values
        assert float(err.max()) < 1e-3, err.tolist()


@pytest.mark.skipif(os.environ.get('SAGECAL_RTR_GRAPH', '1') == '0',
                    reason='RTR graph path is opt-in '
                           '(SAGECAL_RTR_GRAPH=1); round-2 validation')
def test_rtr_graphed_matches_eager():
    """Graph-captured RTR vs the eager solver on the same problem
    (enable with SAGECAL_RTR_GRAPH=1)."""
    from sagecal_amd.solvers import rtr as rtr_mod, lm as lm_mod
    from sagecal_amd.ops.hip_host import BaselineLayout
    from sagecal_amd.ops import reference as R
    dev = 'cuda:0'
    rng = np.random.default_rng(2)
    N, T = 64, 4
    pairs = [(p, q) for p in range(N) for q in range(p + 1, N)]
    Nbase = len(pairs)
    bb = torch.tensor(pairs * T, device=dev)
    B = Nbase * T
    s = torch.tensor(rng.standard_normal(B) + 1j * rng.standard_normal(B))
    coh = (s[:, None, None] * torch.eye(2, dtype=torch.complex128)) \
        .to(device=dev, dtype=torch.complex64)
    Jt = torch.tensor(np.eye(2)[None, None] + 0.2 * (
        rng.standard_normal((1, N, 2, 2))
        + 1j * rng.standard_normal((1, N, 2, 2)))).to(
            device=dev, dtype=torch.complex64)
    x = R.apply_jones(coh.cpu().to(torch.complex128),
                      Jt.cpu().to(torch.complex128), bb.cpu()).to(
                          device=dev, dtype=torch.complex64)
    lay = BaselineLayout(bb, Nbase, T, 1, N, dev)
    prob = lm_mod.LMProblem(x, coh, bb, N, 1, None, layout=lay)
    J0 = Jt + 0.05 * torch.randn_like(Jt.real).to(Jt.dtype)
    os.environ['SAGECAL_RTR_GRAPH'] = '0'
    J_e, info_e = rtr_mod.rtr_solve(prob, J0.clone(), maxiter=10)
    os.environ['SAGECAL_RTR_GRAPH'] = '1'
    J_g, info_g = rtr_mod.rtr_solve_graphed(prob, J0.clone(), maxiter=10)
    ce = float(info_e['final_cost'].max())
    cg = float(info_g['final_cost'].max())
    assert cg <= 1.2 * ce + 1e-6, (ce, cg)


@pytest.mark.skipif(os.environ.get('SAGECAL_BEAM_KERNEL_TEST') != '1',
                    reason='fused beam kernel written round 2, '
                           'GPU-validated next round '
                           '(SAGECAL_BEAM_KERNEL_TEST=1)')
def test_fused_beam_predict_matches_torch():
    """k_predict_coh with the beam argument (-B 1 fused path,
    predict_model.cu:843-852 semantics) vs the torch loop on CPU."""
    from sagecal_amd import sky, beams
    from sagecal_amd.ops.reference import SourcePack
    dev = 'cuda:0'
    srcs, clist = sky.make_synthetic_sky(M=2, nsrc_per_cluster=3, seed=3)
    clusters = sky.build_clusters(srcs, clist, 0.0, np.pi / 4, 150e6)
    pack = SourcePack(clusters)
    N, T = 8, 2
    Nbase = N * (N - 1) // 2
    rng = np.random.default_rng(4)
    B = Nbase * T
    u = torch.tensor(rng.uniform(-1e-5, 1e-5, B))
    v = torch.tensor(rng.uniform(-1e-5, 1e-5, B))
    w = torch.zeros(B, dtype=torch.float64)
    bb = torch.tensor([(p_, q_) for p_ in range(N)
                       for q_ in range(p_ + 1, N)] * T)
    tmjd = np.array([57000.0, 57000.0001])
    rng2 = np.random.default_rng(7)
    elems = [rng2.uniform(-30, 30, (16, 3)) for _ in range(N)]
    cfg = beams.ArrayConfig(elems, 0.1, 0.92, 0.0, np.pi / 4)
    args = (pack, u, v, w, 150e6, 150e6, 1e4, 1.0, np.pi / 4, cfg, tmjd,
            bb, Nbase, T)
    cpu = beams.predict_coh_withbeam(*args, mode=1)
    gargs = (pack, u.to(dev), v.to(dev), w.to(dev), 150e6, 150e6, 1e4,
             1.0, np.pi / 4, cfg, tmjd, bb.to(dev), Nbase, T)
    gpu = beams.predict_coh_withbeam(*gargs, mode=1)
    err = float((gpu.cpu().to(cpu.dtype) - cpu).abs().max()
                / cpu.abs().max())
    assert err < 2e-4, err


@pytest.mark.skipif(os.environ.get('SAGECAL_CHOL_BIG') == '0',
                    reason='opted out via SAGECAL_CHOL_BIG=0')
def test_chol_mw_large_n4096():
    """Chunked-panel mw Cholesky at the 512-station LM shape
    (8N=4096, clmfit_cuda.c:1624-1674 role) vs torch.cholesky_solve."""
    from sagecal_amd.ops.hip_host import chol_solve_damped
    dev = 'cuda:0'
    torch.manual_seed(5)
    n, batch = 4096, 2
    G = torch.randn(batch, n, n, device=dev) / n ** 0.5
    A = G @ G.transpose(-1, -2) + 0.5 * torch.eye(n, device=dev)
    b = torch.randn(batch, n, device=dev)
    mu = torch.full((batch,), 0.1, device=dev)
    # the copy to the host synchronises: a fault in the kernel sequence
    # is reported on this line
    dp = chol_solve_damped(A, b, mu).double().cpu()
    # fp64 reference on the host: with the reference on the device this
    # test died with a launch failure reported at torch's batched fp64
    # cholesky_solve, after torch.linalg.cholesky had synchronised. The
    # cause of that failure is not established; the host reference only
    # keeps torch's device solve out of the test
    Ad = A.double().cpu() + mu.double().cpu()[:, None, None] * torch.eye(
        n, dtype=torch.float64)
    L = torch.linalg.cholesky(Ad)
    ref = torch.cholesky_solve(b.double().cpu().unsqueeze(-1), L).squeeze(-1)
    err = (dp - ref).abs().max() / ref.abs().max()
    assert float(err) < 5e-2, float(err)   # fp32 kernel vs fp64 at n=4096
